"""Records what the reference's own kernels return (oracle/_ref/ref60 and ref30, built by `make -C oracle ref`) for the requests of
tests/ref_words_cases.py, into tests/golden/ref_words.npz.  Needs an MI355X and the built binaries; run from the repository root:

    python tests/golden/make_ref_words.py [OUTPUT.npz]

Per case the fixture holds the first 128 bits of the SHA-256 of the response and, for the small decisive cases, the response or its head
(Item.full); the inputs are not stored -- tests/test_reference_words_host.py re-derives them, runs the oracle alone and compares.  For
the samplers and the complete drivers it also keeps where the reference's three Gaussian polynomials differ from the oracle's own sampler (the one step
whose words the oracle does not claim), as (polynomial, index, value) rows.
"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import oracle_py as oracle          # noqa: E402
import ref_py as R                  # noqa: E402
import ref_words_cases as C         # noqa: E402


def sha(words):
    """the first 16 bytes of the SHA-256 of the little-endian words"""
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(words).astype("<u8").tobytes()).digest()[:16], dtype=np.uint8)


def main(argv):
    out_path = argv[1] if len(argv) > 1 else os.path.join(HERE, "ref_words.npz")
    assert R.available(), R.SKIP_REASON
    oracle.build()
    store, names, digests = {}, [], []
    for gname, make in C.groups(oracle):
        binary, items = make()
        outs = R.run(binary, [it.case for it in items])
        for it, w in zip(items, outs):
            key = "%s/%s" % (gname, it.name)
            names.append(key)
            digests.append(sha(w))
            part = it.stored_part(w)
            if len(part):
                store["words/" + key] = part
        if gname == "samplers":
            inp = C.samplers(oracle)[2]
            store["gauss_diff/samplers"] = C.gauss_diff(C.sampler_gauss_from_responses(items, outs, inp["n"], inp["qs"]),
                                                        C.sampler_gauss_oracle(oracle, inp["n"], inp["qs"], inp["gw"]))
        if gname == "drivers":
            for sname, gauss in C.driver_gauss_from_responses(items, outs).items():
                n, qs = next((it.meta["n"], it.meta["qs"]) for it in items if it.meta["set"] == sname)
                store["gauss_diff/" + sname] = C.gauss_diff(gauss, C.driver_gauss_oracle(oracle, n, qs))
        print("%-18s %3d cases  %8d words" % (gname, len(items), sum(w.size for w in outs)), flush=True)
    store["names"] = np.array(names)
    store["sha256_128"] = np.stack(digests)
    np.savez_compressed(out_path, **store)
    print("wrote %s: %d cases, %d bytes" % (out_path, len(names), os.path.getsize(out_path)))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
