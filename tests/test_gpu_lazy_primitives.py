"""GPU: the lazy primitives of csrc/ntt_core.cuh at the edges of their promised ranges, one `lazy_probe run` per modulus.

tests/cpp/lazy_probe.hip runs one bounds-checked element-wise kernel per op on the crafted operands of tests/lazy_inputs.py (what they
reach is proved on the CPU in tests/test_lazy_bounds_host.py); every word that comes back is held against the CONTRACT of its primitive
(tests/lazy_model.py): the exact value for mul_hi, mul_wide, barrett_mul, lit_barrett_mul (the oracle's singleBarrett word, q + r
included), congruence mod q AND the promised interval for the lazy products, reductions and the fold, the canonical exact value for
canon_after_* and FusedMul -- for class HL_LIT the oracle's word, and for the near-2^k classes with 4q of headroom, whose fold product
hands [0, 2q) to the inverse's first round, congruence and [0, 2q)."""
import os
import subprocess

import pytest

import lazy_inputs as li
import lazy_model as lm

MODULI = li.moduli()


@pytest.mark.gpu
@pytest.mark.parametrize("idx", range(len(MODULI)), ids=[nm for nm, _ in MODULI])
def test_primitives_keep_their_contracts(native, oracle, gpu, tmp_path, idx):
    name, q = MODULI[idx]
    recs, tuples = li.records_for(q)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    lm.write_probe_input(fin, recs)
    r = subprocess.run([lm.build_probe(), "run", fin, fout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    res = lm.read_probe_output(fout, recs)
    L = oracle.lib()
    bad = []
    for (op, hl, near, c, _), tup, got in zip(recs, tuples, res):
        assert len(tup) == len(got), (name, op)
        for i, (t, g) in enumerate(zip(tup, got)):
            msg = lm.contract(op, c, t, g, hl, near)
            if msg is None and i % 5 == 0 and (op in ("barrett_mul", "lit_barrett_mul") or (op == "fused_mul" and hl == lm.HL_LIT)):
                if g != L.orc_barrett(t[0], t[1], q, c["mu"], c["k"]):           # the oracle itself, not only its restatement
                    msg = "oracle's word differs"
            if msg is not None:
                bad.append((op, hl, near, t, g, msg))
    assert not bad, (name, q, len(bad), bad[:5])
