"""GPU: no evaluator call writes past mi355ntt_bfv_eval_scratch_bytes.  The other tests hand every call a buffer of exactly that size,
where a region running past the end would go unnoticed; here the scratch is the start of a larger tensor whose tail, a guard of 4 n
sentinel words, must survive every call, and every output must equal, word for word, that of the same call on a separately allocated
scratch of twice the size.  n = 2048, count = 3 (odd: the two-ciphertexts-per-thread kernels run their tail), r = 6 and 7 either side of
the point where r^2 + 2 r overtakes 8 r + 4, r = 1 and 15 with the largest and the smallest hoist group."""
import numpy as np
import pytest

from bfv_sweep_inputs import demo_subset
from test_gpu_bfv_eval import SENT, sentinel
from test_gpu_bfv_eval_sweep import Sch

GROUPS = {1: 8, 6: 3, 7: 2, 15: 2}                  # include/mi355ntt.h, mi355ntt_bfv_hoist_group


@pytest.mark.gpu
@pytest.mark.parametrize("r", sorted(GROUPS))
def test_calls_stay_inside_scratch_bytes(native, oracle, gpu, r):
    import torch
    n, count = 2048, 3
    qs, psis = demo_subset(n, r)
    S = Sch(native, oracle, n, qs, psis, 1024)
    ev, R = S.ev, S.R
    assert ev.scratch_bytes(count) == (max(8 * r + 4, r * r + 2 * r) + 3 * (r + 1)) * count * n * 8
    assert ev.hoist_group == GROUPS[r]
    words, guard = ev.scratch_bytes(count) // 8, 4 * n
    tight = torch.full((words + guard,), SENT, dtype=torch.int64, device="cuda")
    roomy = torch.full((2 * words,), SENT, dtype=torch.int64, device="cuda")

    d_a = native.to_device(S.encrypt(S.messages(count)))
    d_b = native.to_device(S.encrypt(S.messages(count)))
    d_m = native.to_device(S.messages(count))
    d_mhat = torch.zeros(count * r * n, dtype=torch.int64, device="cuda")
    ev.plain_ntt(d_mhat, d_m, count)
    d_c3 = sentinel(native, 3 * count * R * n)
    ev.multiply(d_c3, d_a, d_b, count)
    gs = [3, n + 1, 3, 2 * n - 1, 5, 25, 2 * n - 3, 1, 5][: GROUPS[r] + 1]      # more elements than one scratch group
    G = len(gs)
    d_gk = torch.zeros(G * r * 2 * R * n, dtype=torch.int64, device="cuda")
    for k, g in enumerate(gs):
        ev.galois_keygen(d_gk[k * r * 2 * R * n:], S.d_sk, g, native.to_device(S.a), native.to_device(S.e))
    d_w = torch.zeros(G * r * n, dtype=torch.int64, device="cuda")
    ev.plain_ntt(d_w, native.to_device(S.messages(G)), G)
    ct = 2 * count * R * n
    calls = [
        ("multiply", 3 * count * R * n, lambda o, s: ev.multiply(o, d_a, d_b, count, scratch=s)),
        ("relinearize", ct, lambda o, s: ev.relinearize(o, d_c3, S.d_rlk, count, scratch=s)),
        ("multiply_relin", ct, lambda o, s: ev.multiply_relin(o, d_a, d_b, S.d_rlk, count, scratch=s)),
        ("multiply_plain", ct, lambda o, s: ev.multiply_plain(o, d_a, d_m, count, scratch=s)),
        ("multiply_plain_ntt", ct, lambda o, s: ev.multiply_plain_ntt(o, d_a, d_mhat, count, scratch=s)),
        ("multiply_plain_ntt shared", ct, lambda o, s: ev.multiply_plain_ntt(o, d_a, d_mhat[: r * n], count, shared=True, scratch=s)),
        ("apply_galois", ct, lambda o, s: ev.apply_galois(o, d_a, d_gk[: r * 2 * R * n], gs[0], count, scratch=s)),
        ("apply_galois_hoisted", G * ct, lambda o, s: ev.apply_galois_hoisted(o, d_a, d_gk, gs, count, scratch=s)),
        ("galois_sum", ct, lambda o, s: ev.galois_sum(o, d_a, d_gk, gs, count, scratch=s)),
        ("galois_sum weighted", ct, lambda o, s: ev.galois_sum(o, d_a, d_gk, gs, count, weights=d_w, scratch=s)),
    ]
    for what, size, call in calls:
        got, want = sentinel(native, size), sentinel(native, size)
        tight[:words].fill_(SENT)
        call(got, tight[:words])
        call(want, roomy)
        torch.cuda.synchronize()
        assert np.array_equal(native.to_host(got), native.to_host(want)), (r, what)
        assert bool((tight[words:] == SENT).all()), (r, what, "guard overwritten")
    S.close()
