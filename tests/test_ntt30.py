"""The reference's 30-bit path (old/ntt_30bit.cuh): 32-bit words, one prime."""
import numpy as np
import pytest

from test_ntt30_moduli import exact_forward30

# getParams30, old/NTT/old_design/final/parameter.h:73-115: n -> (q, psi, psiinv, ninv, q_bit)
PARAMS30 = {
    2048: (12931073, 3733, 10610200, 12924759, 24),
    4096: (33538049, 2386, 26102329, 33529861, 25),
    8192: (8716289, 1089, 8196033, 8715225, 24),
    16384: (13664257, 273, 8959348, 13663423, 24),
    32768: (19070977, 377, 16642842, 19070395, 25),
    65536: (13631489, 13, 12582913, 13631281, 24),       # BFV_Scheme/parameter.h:129-136 (old/ntt_30bit.cuh dispatches N = 65536, :271-283,323-331)
}


def exact_forward(a, q, psi, n):
    lg = n.bit_length() - 1
    tab = [pow(psi, int(format(i, "0%db" % lg)[::-1], 2), q) for i in range(n)]
    a = [int(x) for x in a]
    length = 1
    while length < n:
        step = n // (2 * length)
        for p in range(length):
            w = tab[length + p]
            for j in range(2 * p * step, 2 * p * step + step):
                u, v = a[j], a[j + step] * w % q
                a[j], a[j + step] = (u + v) % q, (u - v) % q
        length *= 2
    return np.array(a, dtype=np.uint32)


@pytest.mark.parametrize("n", sorted(PARAMS30))
def test_oracle30_is_pinned_on_reference_parameters(oracle, n):
    q, psi, psiinv, ninv, bits = PARAMS30[n]
    prm = oracle.Params30(n, q, psi)
    assert (prm.k, prm.psiinv) == (bits, psiinv) and pow(n, -1, q) == ninv and pow(psi, n, q) == q - 1
    rng = np.random.default_rng(n)
    a = rng.integers(0, q, size=n, dtype=np.uint32)
    a[:4] = [0, 1, q - 1, q - 2]
    A = oracle.forward30(a, prm)
    if n <= 4096:
        assert np.array_equal(A, exact_forward(a, q, psi, n))          # the transform the reference means
    assert np.array_equal(A, exact_forward30(a, q, psi, n))            # (the vectorised one at every size)
    assert np.array_equal(oracle.inverse30(A, prm), a)                  # halving butterflies fold n^-1 in
    if n == 2048:                                                       # 30bit_ntt_test.cu's check: schoolbook product
        b = rng.integers(0, q, size=n, dtype=np.uint32)
        c = oracle.inverse30(oracle.pointwise30(A, oracle.forward30(b, prm), prm), prm)
        want = oracle.ref_polymul(a.astype(np.uint64), b.astype(np.uint64), q)
        assert np.array_equal(c.astype(np.uint64), want)


@pytest.mark.gpu
@pytest.mark.parametrize("n", sorted(PARAMS30))
def test_gpu_30bit_path_matches_oracle(native, oracle, gpu, n):
    import torch
    q, psi, _, _, bits = PARAMS30[n]
    prm = oracle.Params30(n, q, psi)
    num = 5
    rng = np.random.default_rng(7 * n)
    a = rng.integers(0, q, size=(num, n), dtype=np.uint32)
    b = rng.integers(0, q, size=(num, n), dtype=np.uint32)
    a[0, :4] = [0, 1, q - 1, q - 2]
    dev32 = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.int32)).to(gpu)
    host32 = lambda t: t.cpu().numpy().view(np.uint32)
    d_a, d_b = dev32(a), dev32(b)
    d_psi, d_psiinv = dev32(prm.psi_tab), dev32(prm.psiinv_tab)
    native.forward30(d_a, n, q, prm.mu, bits, d_psi, num)
    native.forward30(d_b, n, q, prm.mu, bits, d_psi, num)
    torch.cuda.synchronize()
    A, B = oracle.forward30(a, prm), oracle.forward30(b, prm)
    assert np.array_equal(host32(d_a), A) and np.array_equal(host32(d_b), B)
    native.barrett30(d_a, d_b, q, prm.mu, bits)
    AB = oracle.pointwise30(A, B, prm)
    assert np.array_equal(host32(d_a), AB)
    native.inverse30(d_a, n, q, prm.mu, bits, d_psiinv, num)
    assert np.array_equal(host32(d_a), oracle.inverse30(AB, prm))
    native.inverse30(d_b, n, q, prm.mu, bits, d_psiinv, num)
    assert np.array_equal(host32(d_b), b)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [4096, 32768, 65536])
def test_gpu_30bit_literal_fallbacks_match_oracle(native, oracle, gpu, n):
    """The native 30-bit kernels are taken only for the canonical mu and a table of residues; a hand-made mu runs the
    literal kernels from the host side, a table entry >= q is caught on the device (the companion pass in front of every
    call) and sends the call to the literal leg: both must give the words of the oracle's literal arithmetic."""
    import torch
    q, psi, _, _, bits = PARAMS30[n]
    prm = oracle.Params30(n, q, psi)
    num = 3
    rng = np.random.default_rng(11 * n)
    a = rng.integers(0, q, size=(num, n), dtype=np.uint32)
    dev32 = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.int32)).to(gpu)
    host32 = lambda t: t.cpu().numpy().view(np.uint32)
    d_psi, d_psiinv = dev32(prm.psi_tab), dev32(prm.psiinv_tab)
    # (1) mu one too small
    prm2 = oracle.Params30(n, q, psi)
    prm2.mu -= 1
    d_a = dev32(a)
    native.forward30(d_a, n, q, prm2.mu, bits, d_psi, num)
    A2 = oracle.forward30(a, prm2)
    assert np.array_equal(host32(d_a), A2)
    native.inverse30(d_a, n, q, prm2.mu, bits, d_psiinv, num)
    assert np.array_equal(host32(d_a), oracle.inverse30(A2, prm2))
    # (2) a table entry q + w instead of w (same residue, not canonical): the literal arithmetic on exactly that table
    prm3 = oracle.Params30(n, q, psi)
    prm3.psi_tab = prm3.psi_tab.copy()
    prm3.psi_tab[n // 2 + 3] += q
    d_a = dev32(a)
    native.forward30(d_a, n, q, prm3.mu, bits, dev32(prm3.psi_tab), num)
    assert np.array_equal(host32(d_a), oracle.forward30(a, prm3))
    # (3) and the clean table right afterwards on the same stream: the native kernels again
    d_a = dev32(a)
    native.forward30(d_a, n, q, prm.mu, bits, d_psi, num)
    assert np.array_equal(host32(d_a), oracle.forward30(a, prm))


def test_30bit_entry_points_reject_bad_arguments(native):
    L = native.lib()
    assert L.mi355ntt_forward30_raw(None, 2048, None, 12931073, 21767333, 24, None) == native.EINVAL
    assert L.mi355ntt_forward30_batch_raw(native.vp(16), 1000, native.vp(16), 1, 12931073, 21767333, 24, None) == native.EUNSUPPORTED
    assert L.mi355ntt_barrett30_raw(native.vp(16), native.vp(16), 8, 1 << 31, 5, 31, None) == native.EUNSUPPORTED


@pytest.mark.gpu
@pytest.mark.parametrize("n,num", [(32768, 601), (4096, 2500), (65536, 301), (2048, 4500)])
def test_gpu_30bit_persistent_loop_matches_oracle(native, oracle, gpu, n, num):
    """more polynomials than resident workgroups: every workgroup of the native kernels walks several polynomials (prefetch
    of the next one in a second register set, zero-length prefetch past the end, middle-round twiddles resident in LDS at
    n = 2^15); every word of forward and inverse against the oracle"""
    import torch
    q, psi, _, _, bits = PARAMS30[n]
    prm = oracle.Params30(n, q, psi)
    rng = np.random.default_rng(11 * n)
    a = rng.integers(0, q, size=(num, n), dtype=np.uint32)
    dev32 = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.int32)).to(gpu)
    host32 = lambda t: t.cpu().numpy().view(np.uint32)
    d_a = dev32(a)
    d_psi, d_psiinv = dev32(prm.psi_tab), dev32(prm.psiinv_tab)
    native.forward30(d_a, n, q, prm.mu, bits, d_psi, num)
    torch.cuda.synchronize()
    A = oracle.forward30(a, prm)
    assert np.array_equal(host32(d_a), A)
    native.inverse30(d_a, n, q, prm.mu, bits, d_psiinv, num)
    torch.cuda.synchronize()
    assert np.array_equal(host32(d_a), a)


@pytest.mark.gpu
@pytest.mark.parametrize("num", [31, 32, 100, 129, 383, 384, 420])
def test_gpu_30bit_n65536_pair_launch_matches_oracle(native, oracle, gpu, num):
    """n = 65536 (old/ntt_30bit.cuh:271-283,323-331), large calls (forward from 32, inverse from 384 polynomials): no stage launch,
    two cooperating workgroups per polynomial (k_ntt30x PAIR).  Forward: both read both halves and keep one half of the first stage's output each, one "have
    read it" flag each way before the in-place stores.  Inverse: the upper workgroup writes its half-size result through and
    counts it, the lower one reads it back and stores both halves of the last stage's output.  Either side of the switch, odd and even grids (partners on different / the
    same XCD), workgroups with a second polynomial; adversarial words; then a table with an entry >= q behind the same
    launch (the native kernel steps aside on the device, the literal leg runs every stage), two streams at once, and a
    captured graph (capturing streams keep the stage launch)."""
    import torch
    n = 65536
    q, psi, _, _, bits = PARAMS30[n]
    prm = oracle.Params30(n, q, psi)
    rng = np.random.default_rng(num)
    a = rng.integers(0, q, size=(num, n), dtype=np.uint32)
    a[0, :4] = [0, q - 1, 1, q - 1]
    a[0, n // 2 - 2: n // 2 + 2] = q - 1
    a[num - 1, :] = q - 1
    dev32 = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.int32)).to(gpu)
    host32 = lambda t: t.cpu().numpy().view(np.uint32)
    d_psi, d_psiinv = dev32(prm.psi_tab), dev32(prm.psiinv_tab)
    A = oracle.forward30(a, prm)
    d_a = dev32(a)
    native.forward30(d_a, n, q, prm.mu, bits, d_psi, num)
    assert np.array_equal(host32(d_a), A)
    native.inverse30(d_a, n, q, prm.mu, bits, d_psiinv, num)
    assert np.array_equal(host32(d_a), a)
    if num not in (32, 129, 420):
        return
    # a table entry q + w (same residue, not canonical): the literal arithmetic on exactly that table, then the clean table again
    prm3 = oracle.Params30(n, q, psi)
    prm3.psi_tab = prm3.psi_tab.copy()
    prm3.psi_tab[1] += q                             # (the entry of the stage that couples the halves)
    small = a[:num]
    d_b = dev32(small)
    native.forward30(d_b, n, q, prm3.mu, bits, dev32(prm3.psi_tab), num)
    assert np.array_equal(host32(d_b), oracle.forward30(small, prm3))
    d_b = dev32(a)
    native.forward30(d_b, n, q, prm.mu, bits, d_psi, num)
    assert np.array_equal(host32(d_b), A)
    # the same for the inverse (pair launch: the upper workgroup hands its half-size result to the lower one, which applies the
    # last stage): entry 1 of the inverse table not canonical -> literal leg, every stage; then the clean table again
    prm4 = oracle.Params30(n, q, psi)
    prm4.psiinv_tab = prm4.psiinv_tab.copy()
    prm4.psiinv_tab[1] += q
    d_b = dev32(A)
    native.inverse30(d_b, n, q, prm4.mu, bits, dev32(prm4.psiinv_tab), num)
    assert np.array_equal(host32(d_b), oracle.inverse30(A, prm4))
    d_b = dev32(A)
    native.inverse30(d_b, n, q, prm.mu, bits, d_psiinv, num)
    assert np.array_equal(host32(d_b), a)
    # two streams, nobody waits (each stream has its own scratch table and flags)
    d_c, d_d = dev32(a), dev32(a)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    for _ in range(2):
        native.forward30(d_c, n, q, prm.mu, bits, d_psi, num, stream=s1)
        native.forward30(d_d, n, q, prm.mu, bits, d_psi, num, stream=s2)
        native.inverse30(d_c, n, q, prm.mu, bits, d_psiinv, num, stream=s1)
        native.inverse30(d_d, n, q, prm.mu, bits, d_psiinv, num, stream=s2)
    native.forward30(d_c, n, q, prm.mu, bits, d_psi, num, stream=s1)
    native.forward30(d_d, n, q, prm.mu, bits, d_psi, num, stream=s2)
    torch.cuda.synchronize()
    # (the second stream finds the pair slot held and takes the stage launch NEXT to the first stream's pair launch.  Its very first call
    # also allocates the stream's scratch table: until round 6 the table's guard words were zeroed by a hipMemset on the null stream,
    # which could land AFTER the call's prepare kernel on a busy device -- inside the full suite this assertion failed, never alone)
    assert np.array_equal(host32(d_c), A), "two streams: first stream"
    assert np.array_equal(host32(d_d), A), "two streams: second stream"
    # captured (the first call on the capture stream happens outside the capture: it allocates the stream's scratch table)
    cs = torch.cuda.Stream()
    d_e = dev32(a)
    native.forward30(d_e, n, q, prm.mu, bits, d_psi, num, stream=cs)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=cs):
        native.inverse30(d_e, n, q, prm.mu, bits, d_psiinv, num)
        native.forward30(d_e, n, q, prm.mu, bits, d_psi, num)
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(host32(d_e), A)
