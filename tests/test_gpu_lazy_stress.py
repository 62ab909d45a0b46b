"""GPU: the stress polynomials of the lazy transforms through NTTContext against the oracle, word for word.

forward_batch, inverse_batch, polymul_batch and polymul_batch_shared (group 0) for every entry of tests/lazy_stress.py (the class forms of
KERNEL_FORMS and the tightest modulus of every lazy class), on both sides of the small-batch switch, the polynomials cycled through the
batch so that every workgroup of a persistent launch sees one.

n = 2048 and 4096: the committed winners of the hill-climb on the whole-transform model (tests/golden/lazy_stress_*.npz: largest value /
2^64 and smallest margin of forward, inverse and product; tests/test_lazy_bounds_host.py re-runs the model on them) and the model-free
seeds.  n = 8192 ... 65536: the same coefficient PATTERNS -- all q - 1, alternating 0 / q - 1, a single q - 1 at 0, 1, n/2, n - 1, the
back-solves whose exact transform (the oracle's) is all q - 1, the forward stage-state back-solves of the reducing stages -- without a
model behind them: the model's peaks are only claimed for n <= 4096."""
import numpy as np
import pytest

import lazy_stress as ls

fz = ls.fz
ENTRIES = ls.entries()
SIZES = (2048, 4096, 8192, 16384, 32768, 65536)


def _patterns(oracle, prm, entry, n, psi):
    _, q, hl, near = entry
    if n in ls.MODEL_SIZES:
        return {op: ls.crafted_set(entry, n, op) for op in ls.OPS}
    return ls.large_patterns(q, psi, n, hl, lambda a: oracle.forward(a, prm, 0), lambda a: oracle.inverse(a, prm, 0))


# (a modulus of KERNEL_FORMS need only be 1 mod 2^16: it has no ring of n = 2^16)
CASES = [(e, n) for e in ENTRIES for n in SIZES if (e[1] - 1) % (2 * n) == 0]


@pytest.mark.gpu
@pytest.mark.parametrize("entry,n", CASES, ids=["%s-%d" % (e[0], n) for e, n in CASES])
def test_stress_polynomials_match_the_oracle(native, oracle, gpu, entry, n):
    import torch
    name, q, hl, near = entry
    psi = fz.psi_for(q, n)                      # (the root the fixtures were searched with)
    prm = oracle.Params(n, [q], [psi])
    one = oracle.Params(n, [q], [psi], tables=False)
    ctx = native.NTTContext(n, [q], [psi])
    assert ctx.kernel_class == (hl, near) and not ctx.uses_literal_kernels, (name, ctx.kernel_class)
    pats = {op: np.stack([np.asarray(p, dtype=np.uint64) for p in v]) for op, v in _patterns(oracle, prm, entry, n, psi).items()}
    assert all(int(p.max()) < q for p in pats.values())
    bh = np.asarray(ls.bhat(q, n), dtype=np.uint64)
    # the expected words, once per distinct polynomial
    want = {"fwd": np.stack([oracle.forward(p, prm, 0) for p in pats["fwd"]]),
            "inv": np.stack([oracle.inverse(p, prm, 0) for p in pats["inv"]]),
            "mul": np.stack([oracle.inverse(oracle.pointwise_batch(oracle.forward(p, prm, 0), bh, one).reshape(-1), prm, 0)
                             for p in pats["mul"]])}

    def check(what, d, num, op):
        torch.cuda.synchronize()
        got = native.to_host(d).reshape(num, n)
        sel = np.arange(num) % len(pats[op])
        bad = np.nonzero((got != want[op][sel]).any(axis=1))[0]
        assert bad.size == 0, (name, q, n, num, what, "polynomials", bad[:8].tolist(), "patterns", sel[bad[:8]].tolist())

    for num in ls.BATCHES[n]:
        cyc = {op: pats[op][np.arange(num) % len(pats[op])] for op in ls.OPS}
        d = native.to_device(cyc["fwd"])
        ctx.forward_batch(d, num)
        check("forward_batch", d, num, "fwd")
        d = native.to_device(cyc["inv"])
        ctx.inverse_batch(d, num)
        check("inverse_batch", d, num, "inv")
        d = native.to_device(cyc["mul"])
        ctx.polymul_batch(d, native.to_device(np.tile(bh, (num, 1))), num)
        check("polymul_batch", d, num, "mul")
        d = native.to_device(cyc["mul"])
        ctx.polymul_batch_shared(d, native.to_device(bh.reshape(1, n)), num, 1, 0)
        check("polymul_batch_shared", d, num, "mul")
    ctx.close()
