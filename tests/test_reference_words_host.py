"""The oracle against words the reference's own kernels computed (CPU; no GPU and no reference tree needed).

tests/golden/ref_words.npz was recorded on an MI355X by tests/golden/make_ref_words.py from oracle/_ref/ref60 and ref30 -- the reference's
kernels built for gfx950, with only its two inline-PTX functions restated (oracle/ref_shim.h).  Here every input is re-derived
(tests/ref_words_cases.py), the oracle runs alone, and its words must be the recorded ones: the stored words where the fixture keeps them,
the SHA-256 of the whole response everywhere.  tests/test_gpu_reference_words.py is the three-way comparison on the GPU."""
import hashlib
import os

import numpy as np
import pytest

import params as P
import ref_py as R
import ref_words_cases as C

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_words.npz")


def sha(words):
    """the first 128 bits of the SHA-256 of the little-endian words, as the fixture keeps them"""
    return hashlib.sha256(np.ascontiguousarray(words).astype("<u8").tobytes()).digest()[:16]


_GROUPS = {}


def group(oracle, gname):
    """the items of a group, built once per session (several tests walk them)"""
    if gname not in _GROUPS:
        _GROUPS[gname] = dict(C.groups(oracle))[gname]()[1]
    return _GROUPS[gname]


@pytest.fixture(scope="module")
def recorded():
    z = np.load(FIXTURE)
    digests = dict(zip([str(x) for x in z["names"]], [bytes(x) for x in z["sha256_128"]]))
    return z, digests


def test_reference_binaries_are_built_where_the_reference_tree_is():
    """Where the reference tree is on the machine, build() has made all three binaries and none is older than the recipe: a missing
    binary is a failure there, so the GPU tests cannot skip silently on the machine that builds the tree before it travels."""
    if R.reference_tree() is None:
        assert not os.environ.get("REFERENCE"), "REFERENCE is set but holds no BFV_Scheme/"
        return
    for b in R.BINARIES:
        assert os.access(b, os.X_OK), "%s missing although the reference tree is present: run build()" % b
        newest = max(os.path.getmtime(f) for f in R.RECIPE)
        assert os.path.getmtime(b) >= newest, "%s is older than the recipe files" % b
    src = os.path.join(R.REF_DIR, "src")
    assert len([f for f in os.listdir(src) if f.endswith((".cuh", ".h"))]) == 10 and os.path.exists(os.path.join(src, "ref30", "ntt_30bit.cuh"))


def test_fixture_names_are_the_cases(oracle, recorded):
    _, digests = recorded
    want = ["%s/%s" % (g, it.name) for g in C.GROUP_NAMES for it in group(oracle, g)]
    assert sorted(want) == sorted(digests) and len(set(want)) == len(want)


@pytest.mark.parametrize("gname", [g for g in C.GROUP_NAMES if g != "drivers"])
def test_oracle_returns_the_recorded_reference_words(oracle, recorded, gname):
    z, digests = recorded
    items = group(oracle, gname)
    claimed = 0
    for it in items:
        key = "%s/%s" % (gname, it.name)
        if it.expect is None:
            continue
        want = it.expect()
        if it.full:
            rec = z["words/" + key]
            got = it.stored_part(want)
            bad = np.nonzero(rec != got)[0]
            assert rec.shape == got.shape and bad.size == 0, (key, bad[:8], [(hex(int(rec[i])), hex(int(got[i]))) for i in bad[:4]])
        assert sha(want) == digests[key], key
        claimed += 1
        if it.meta.get("class0") and it.meta["op"] == "forward":          # the case tells class 0 from an exact transform: some word is q + r, which no exact kernel returns
            assert (want >= np.uint64(it.meta["q"])).any(), key
        if it.meta.get("op") == "barrett" and it.meta["noncanonical"]:
            assert int((want >= np.uint64(it.meta["q"])).sum()) >= it.meta["noncanonical"], key
    assert claimed >= len(items) - 2


def test_class0_cases_cover_every_inexact_prime(oracle):
    """every (n, inexact prime) of the transform groups has an input whose reference forward holds a word q + r -- all but the one pair
    for which neither a drawn nor a constructed input exists -- and the pointwise group reaches q + r on every inexact prime"""
    for n in C.SIZES:
        have = {it.meta["q"] for it in group(oracle, "transforms-n%d" % n) if it.meta.get("class0") and it.meta["op"] == "forward"}
        want = {q for q, _ in C.inexact_moduli(n) if (n, q) not in C.NOT_CONSTRUCTED}
        assert have == want, (n, want - have)
    assert C.NOT_CONSTRUCTED == {(4096, P.INEXACT_PRIMES[36][0])}
    inexact = {v[0] for v in P.INEXACT_PRIMES.values()}
    for it in group(oracle, "pointwise"):
        if it.meta["op"] == "barrett":
            assert (it.meta["noncanonical"] > 0) == (it.meta["q"] in inexact), it.name


def test_gaussian_words_of_the_reference_against_the_oracle(oracle, recorded):
    """The oracle's inverse normal CDF is AS241, the device's is normcdfinvf.  The fixture keeps every word on which the reference binary
    differed from the oracle (gauss_diff); the oracle's polynomials corrected by those rows reproduce the recorded responses of
    gaussian_dist_xq and convert_ternary_gaussian_x2 (digest; the ternary half is the oracle's exactly), and go through check_gaussian,
    the criterion test_gpu_bfv_launch_edges.py applies to the library, unchanged."""
    from test_gpu_bfv_launch_edges import check_gaussian
    z, digests = recorded
    _, items, inp = C.samplers(oracle)
    n, qs, gw = inp["n"], inp["qs"], inp["gw"]
    diff = z["gauss_diff/samplers"]
    print("Gaussian words where the reference binary differs from the oracle (polynomial, index, value):", diff.tolist())
    ref = [C.residues(g, qs, n) for g in C.gauss_patched(C.sampler_gauss_oracle(oracle, n, qs, gw), diff)]
    for k in range(3):
        check_gaussian(ref[k], oracle.sample_xq("gaussian", gw[k].view(np.uint8), n, qs), gw[k], qs)
    tern = oracle.sample_xq("ternary", inp["tern"], n, qs)
    name = {it.meta["op"]: "samplers/" + it.name for it in items}
    assert sha(ref[0].reshape(-1)) == digests[name["gaussian"]]
    assert sha(np.concatenate([tern.reshape(-1), tern.reshape(-1), ref[1].reshape(-1), ref[2].reshape(-1)])) == digests[name["convert_x2"]]


def test_oracle_drivers_return_the_recorded_reference_words(oracle, recorded):
    """keygen_rns -> encryption_rns -> decryption_rns by the oracle from the reference's keystream, its Gaussian polynomials corrected wherever the fixture records the reference's to differ:
    secret key, public key, ciphertext and the whole buffer after decryption are the reference binary's; the plaintext is the message."""
    from test_gpu_bfv_launch_edges import check_gaussian
    z, digests = recorded
    for it in group(oracle, "drivers"):
        if it.meta["op"] != "drivers":
            continue
        n, qs, psis, t, gamma = (it.meta[k] for k in ("n", "qs", "psis", "t", "gamma"))
        diff = z["gauss_diff/" + it.meta["set"]]
        print(it.name, "Gaussian words where the reference binary differs from the oracle:", diff.tolist())
        gauss = C.gauss_patched(C.driver_gauss_oracle(oracle, n, qs), diff)
        d = C.drivers_oracle(oracle, n, qs, psis, t, gamma, gauss)
        assert sha(np.concatenate([d["sk"], d["pk"], d["c_enc"], d["c_dec"]])) == digests["drivers/" + it.name], it.name
        assert np.array_equal(d["plain"], d["m"]) and np.array_equal(d["c_dec"][n * (len(qs) - 2): n * (len(qs) - 1)], d["m"])
        Rn, ks = len(qs), d["keystream"]
        streams = (ks[n + 8 * Rn * n: n + 8 * Rn * n + 4 * n], ks[n: 5 * n], ks[5 * n: 9 * n])
        for small, by in zip(gauss, streams):
            check_gaussian(C.residues(small, qs, n), oracle.sample_xq("gaussian", by, n, qs), np.ascontiguousarray(by).view(np.uint32), qs)
