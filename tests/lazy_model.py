"""The lazy arithmetic of csrc/ntt_core.cuh stated three ways (test infrastructure).

1. CONTRACTS in Python integers -- what each primitive promises (the congruence mod q and the interval, or the exact value), never how
   it gets there.  These are the expected values of tests/test_gpu_lazy_primitives.py.
2. A WORD-EXACT RESTATEMENT of the algorithms on numpy uint64 words (the three-product quotient, the reciprocal estimate, the fold,
   the ct_round / gs_round butterflies with the masks and cmul read from `lazy_probe policy`, IN2Q, the class-2 / class-3 conditional
   subtractions, fin_red).  It is used ONLY to classify and to search for inputs -- which band and quotient error an operand reaches,
   how high a transform's lazy values climb, how small the margins get -- never as an expected value.
3. An INTERVAL CHECKER of the policy: from the primitives' promised output ranges alone, every sum stays below 2^64, every cq covers
   what is subtracted, every value entering a primitive lies in its promised domain.
"""
import json
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE_SRC = os.path.join(ROOT, "tests", "cpp", "lazy_probe.hip")
PROBE_EXE = os.path.join(ROOT, "tests", "cpp", "lazy_probe")
M64 = (1 << 64) - 1
U = np.uint64
HL_LIT = 0

OPS = ["mul_hi", "mul_wide", "barrett_mul", "shoup_mul_lazy", "mul_shoup2", "mul_shoup4m", "mul_shoup4m_tws", "mul_shoup4m_acc",
       "mul_shoup4m_acc_tws", "reduce_2q", "reduce_2q_near", "mul_fold_near", "lit_barrett_mul", "canon_fwd", "canon_inv", "fused_mul"]
OP_ID = {nm: i for i, nm in enumerate(OPS)}
MAGIC = 0x4c415a5950524f42
BLOCK = 64


# ---------------------------------------------------------------------------------------------------------------------------
# the probe
# ---------------------------------------------------------------------------------------------------------------------------
def build_probe():
    deps = [PROBE_SRC] + [os.path.join(ROOT, "ntt-cuda_amd", "csrc", f) for f in ("ntt_core.cuh", "modarith.cuh", "tune.hpp")]
    if not os.path.exists(PROBE_EXE) or os.path.getmtime(PROBE_EXE) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-std=c++17", "-O2", "--offload-arch=gfx950", PROBE_SRC, "-o", PROBE_EXE])
    return PROBE_EXE


_POLICY = None


def probe_policy():
    """`lazy_probe policy` (host only): {(logn, hl): {tq, fwd_mask, inv_mask, cmul}}, the instantiated classes"""
    global _POLICY
    if _POLICY is None:
        r = subprocess.run([build_probe(), "policy"], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stderr
        j = json.loads(r.stdout)
        _POLICY = ({(e["logn"], e["hl"]): e for e in j["policy"]}, [(h, bool(nr)) for h, nr in j["classes"]], j)
    return _POLICY


def probe_consts(q):
    r = subprocess.run([build_probe(), "consts", str(q), str(q.bit_length())], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout)


def policy_py(logn, hl, h_scale=1):
    """fwd_reduce_mask / InvPolicy restated (the host test holds it against the probe's output); h_scale = 2: a deliberately
    unsound policy that believes in twice the headroom"""
    tq = 2 if hl <= 2 else 4
    H = (1 << hl) * h_scale
    fm, B = 0, 1
    for s in range(logn):
        if B + tq > H:
            fm |= 1 << s
            B = 2
        B += tq
    im, cmul, B = 0, [], 1
    for s in range(logn):
        cmul.append(B)
        Bn = max(2 * B, tq)
        if s + 1 < logn and 2 * Bn > H:
            im |= 1 << s
            Bn = max(tq, 2)
        B = Bn
    return {"logn": logn, "hl": hl, "tq": tq, "fwd_mask": fm, "inv_mask": im, "cmul": cmul}


def class_of(q):
    """(HL, NEAR) of a context that holds only q (fast_tables_create, dispatch_class)"""
    c = consts(q)
    hl = min(64 - q.bit_length(), 6)
    if not c["near_ok"] and hl == 5:
        hl = 4
    return hl, c["near_ok"]


# ---------------------------------------------------------------------------------------------------------------------------
# constants of a modulus
# ---------------------------------------------------------------------------------------------------------------------------
def consts(q):
    """prime_reduction_constants restated (the host test holds it against `lazy_probe consts`, i.e. the library's own function)"""
    k = q.bit_length()
    g = min(k - 1, 16)
    d = (1 << k) - q
    near_ok = k > 32 and d < (1 << 24) and (d << (64 - k)) + 2 * d < (1 << k) and 2 * d * d + 3 * d < (1 << k)
    return {"q": q, "k": k, "nq": (1 << 64) - q, "red_sh1": k - 1 - g, "red_sh2": g, "red_c": ((1 << (31 + k)) // q) & 0xffffffff,
            "delta": d if near_ok else 0, "near_sh": k - 32 if k > 32 else 0, "near_mask": (1 << (k - 32)) - 1 if k > 32 else 0,
            "near_ok": near_ok, "mu": (1 << (2 * k)) // q}


def shoup(w, q):
    return (w << 64) // q


# ---------------------------------------------------------------------------------------------------------------------------
# 1. contracts (Python integers)
# ---------------------------------------------------------------------------------------------------------------------------
def single_barrett(a, b, q, mu, k):
    """the reference's mul64 + singleBarrett with its truncations to the low limb (ntt_60bit.cuh:44-61) -- for ANY 64-bit operands"""
    P = a * b
    x1 = (P >> (k - 2)) & M64
    s = ((x1 * mu) >> (k + 2)) & M64
    r = (P - s * q) & M64
    return r - q if r >= q else r


def tq_of(hl):
    return 2 if hl <= 2 else 4


def fused_is_lazy(hl, near):
    return hl != HL_LIT and near and hl > 2


def contract(op, c, args, got, hl=None, near=None):
    """None when `got` (one word; mul_wide: (lo, hi)) keeps the promise of `op` on the operand tuple `args`, else a message"""
    q, k = c["q"], c["k"]

    def lazy(x, value, bound):
        if x % q != value % q:
            return "not congruent"
        if not 0 <= x < bound * q:
            return "outside [0, %dq): %d q + %d" % (bound, x // q, x % q)
        return None

    if op == "mul_hi":
        return None if got == (args[0] * args[1]) >> 64 else "value"
    if op == "mul_wide":
        P = args[0] * args[1]
        return None if got == (P & M64, P >> 64) else "value"
    if op in ("barrett_mul", "lit_barrett_mul"):
        return None if got == single_barrett(args[0], args[1], q, c["mu"], k) else "value"
    if op == "shoup_mul_lazy" or op == "mul_shoup2":
        return lazy(got, args[0] * args[1], 2)
    if op in ("mul_shoup4m", "mul_shoup4m_tws"):
        return lazy(got, args[0] * args[1], 4)
    if op in ("mul_shoup4m_acc", "mul_shoup4m_acc_tws"):            # (y, w, wp, base): product + base, mod 2^64
        return lazy((got - args[3]) & M64, args[0] * args[1], 4)
    if op in ("reduce_2q", "reduce_2q_near"):
        return lazy(got, args[0], 2)
    if op == "mul_fold_near":
        return lazy(got, args[0] * args[1], 2)
    if op in ("canon_fwd", "canon_inv"):
        return None if got == (args[0] if hl == HL_LIT else args[0] % q) else "value"
    if op == "fused_mul":
        if hl == HL_LIT:
            return None if got == single_barrett(args[0], args[1], q, c["mu"], k) else "value"
        if fused_is_lazy(hl, near):         # the fold product hands [0, 2q) to the inverse's first round (IN2Q)
            return lazy(got, args[0] * args[1], 2)
        return None if got == args[0] * args[1] % q else "value"
    raise KeyError(op)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. word-exact restatement (numpy uint64; wrapping arithmetic is the device's)
# ---------------------------------------------------------------------------------------------------------------------------
_M32 = U(0xffffffff)
_S32 = U(32)


def arr(x):
    return np.asarray(x, dtype=np.uint64)


def w_mul_hi(a, b):
    a0, a1, b0, b1 = a & _M32, a >> _S32, b & _M32, b >> _S32
    p00 = a0 * b0
    p01 = a0 * b1 + (p00 >> _S32)
    p10 = a1 * b0 + (p01 & _M32)
    return a1 * b1 + (p01 >> _S32) + (p10 >> _S32)


def w_quot3(y, wp):
    """mul_shoup4m's quotient estimate: three of the four partial products of y * wp"""
    y0, y1, p0, p1 = y & _M32, y >> _S32, wp & _M32, wp >> _S32
    return y1 * p1 + ((y0 * p1) >> _S32) + ((y1 * p0) >> _S32)


def w_quot2(y, wp):
    """the MUTATION of the issue: one more partial product dropped (classification / evidence only)"""
    y0, y1, p1 = y & _M32, y >> _S32, wp >> _S32
    return y1 * p1 + ((y0 * p1) >> _S32)


def w_mul_shoup4m(y, w, wp, q, base=0, quot=w_quot3):
    with np.errstate(over="ignore"):
        return y * w - quot(y, wp) * U(q) + arr(base)


def w_mul_shoup2(y, w, wp, q):
    with np.errstate(over="ignore"):
        return y * w - w_mul_hi(y, wp) * U(q)


def w_reduce_2q(x, c, red_c=None):
    """the reciprocal estimate: (e, x - e q)"""
    t = x >> U(c["red_sh1"])
    assert int(t.max(initial=0)) < (1 << 32), "reduce_2q: the top bits of x do not fit 32 bits"
    e = ((t * U(c["red_c"] if red_c is None else red_c)) >> _S32) >> U(c["red_sh2"])
    with np.errstate(over="ignore"):
        return e, x - e * U(c["q"])


def w_reduce_2q_near(x, c):
    """the fold: (e, (x mod 2^k) + e delta)"""
    e = x >> U(c["k"])
    return e, (x & U((1 << c["k"]) - 1)) + e * U(c["delta"])


def w_mul_fold_near(x, b, c):
    """(F, t, result) of the double fold, from Python integers per element (the 128-bit product)"""
    k, d = c["k"], c["delta"]
    F, T, R = [], [], []
    for xi, bi in zip((int(v) for v in x), (int(v) for v in b)):
        P = xi * bi
        f = (P >> k) * d + (P & ((1 << k) - 1))
        t = f >> k
        F.append(f)
        T.append(t)
        R.append(t * d + (f & ((1 << k) - 1)))
    return F, T, R


def w_reduce_sel(x, c, near):
    return w_reduce_2q_near(x, c)[1] if near else w_reduce_2q(x, c)[1]


def w_csub(x, m):
    return np.where(x >= U(m), x - U(m), x)


def classify_shoup4m(y, w, q):
    """(quotient error of the three-product estimate against floor(y wp / 2^64), band floor(result / q)) per operand"""
    wp = arr([shoup(int(v), q) for v in w])
    h3 = w_quot3(y, wp)
    err = w_mul_hi(y, wp) - h3
    res = w_mul_shoup4m(y, w, wp, q)
    return err, res // U(q), wp


def bitrev(i, bits):
    return int(format(i, "0%db" % bits)[::-1], 2) if bits else 0


class Tables:
    """psi / psi^-1 tables in the reference's order (entry i = psi^bitrev(i)), Shoup companions, n^-1"""

    def __init__(self, q, psi, n):
        self.q, self.n, self.logn = q, n, n.bit_length() - 1
        psiinv = pow(psi, q - 2, q)
        pw, pi = [1] * n, [1] * n
        for i in range(1, n):
            pw[i] = pw[i - 1] * psi % q
            pi[i] = pi[i - 1] * psiinv % q
        br = [bitrev(i, self.logn) for i in range(n)]
        self.fw = [pw[br[i]] for i in range(n)]
        self.iw = [pi[br[i]] for i in range(n)]
        self.ninv = pow(n, q - 2, q)
        self.c = consts(q)
        self.fwd = (arr(self.fw), arr([shoup(w, q) for w in self.fw]))
        self.inv = (arr(self.iw), arr([shoup(w, q) for w in self.iw]))
        iwn = [w * self.ninv % q for w in self.iw]
        self.invn = (arr(iwn), arr([shoup(w, q) for w in iwn]))
        self.idx = np.arange(n, dtype=np.int64)


class Trace:
    """what a model run observed: per stage the largest value / 2^64 and the smallest margins (in units of q)"""

    def __init__(self, q):
        self.q = q
        self.stages = []

    def add(self, name, peak, margin_sub, headroom):
        self.stages.append({"stage": name, "word": peak, "peak": peak / 2.0 ** 64, "peak_q": peak / self.q, "margin": margin_sub, "headroom": headroom})

    @property
    def peak(self):
        return max(s["peak"] for s in self.stages)

    @property
    def peak_word(self):
        """the largest value as an integer (peak is a float and rounds to 1.0 just below 2^64)"""
        return max(s["word"] for s in self.stages)

    @property
    def peak_q(self):
        return max(s["peak_q"] for s in self.stages)

    @property
    def margin(self):
        return min(s["margin"] for s in self.stages)


class Wrapped(AssertionError):
    pass


def _sum_no_wrap(a, b, what):
    with np.errstate(over="ignore"):
        s = a + b
    if bool((s < a).any()):
        raise Wrapped("%s wraps 2^64" % what)
    return s


def model_forward(a, tb, hl, near, trace, in2q_bound=False):
    """canonical coefficients -> the lazy words in front of canon_after_forward (bit-reversed order), as ct_round produces them"""
    pol = probe_policy()[0][(tb.logn, hl)]
    q, c, n, logn = tb.q, tb.c, tb.n, tb.logn
    tq, ex = pol["tq"], hl <= 2
    cq = tq * q
    v = arr(a).copy()
    for s in range(logn):
        bit = logn - 1 - s
        lo = tb.idx[(tb.idx >> bit) & 1 == 0]
        hi = lo + (1 << bit)
        ti = (1 << s) + (lo >> (logn - s))
        Uv = v[lo]
        if (pol["fwd_mask"] >> s) & 1:
            Uv = w_reduce_sel(Uv, c, near)
        w, wp = tb.fwd[0][ti], tb.fwd[1][ti]
        T = w_mul_shoup2(v[hi], w, wp, q) if ex else w_mul_shoup4m(v[hi], w, wp, q)
        if int(T.max()) >= cq:
            raise Wrapped("forward stage %d: product outside [0, %dq)" % (s, tq))
        A = _sum_no_wrap(Uv, T, "forward stage %d: U + T" % s)
        Uc = _sum_no_wrap(Uv, arr(cq), "forward stage %d: U + cq" % s)
        v[lo], v[hi] = A, Uc - T
        peak = max(int(A.max()), int(Uc.max()))
        trace.add("fwd%d" % s, peak, (cq - int(T.max())) / q, (M64 - peak) / q)
    return v


def model_canon_forward(v, tb, hl, near):
    return w_csub(w_reduce_sel(v, tb.c, near), tb.q)


def model_fused_mul(v, b, tb, hl, near):
    """FusedMul<HL, NEAR>::mul on the forward's lazy words; (values, lazy hand-over?)"""
    if fused_is_lazy(hl, near):
        x = w_reduce_2q_near(v, tb.c)[1]
        return arr(w_mul_fold_near(x, b, tb.c)[2]), True
    x = w_csub(w_reduce_sel(v, tb.c, near), tb.q)
    return arr([int(xi) * int(bi) % tb.q for xi, bi in zip(x, b)]), False


def model_inverse(a, tb, hl, near, trace, in2q=False):
    """bit-reversed values (canonical, or below 2q with in2q) -> the lazy words in front of canon_after_inverse, as gs_round produces
    them in the single-pass kernels: n^-1 folded into the twiddles of the last round"""
    pol = probe_policy()[0][(tb.logn, hl)]
    q, c, n, logn = tb.q, tb.c, tb.n, tb.logn
    tq, ex = pol["tq"], hl <= 2
    low5 = 5 * ((logn + 4) // 5 - 1)                     # first stage of the last round
    v = arr(a).copy()
    for beta in range(logn):
        last = beta == logn - 1
        lo = tb.idx[(tb.idx >> beta) & 1 == 0]
        hi = lo + (1 << beta)
        ti = (1 << (logn - 1 - beta)) + (lo >> (beta + 1))
        cm = 2 if (in2q and beta == 0) else pol["cmul"][beta]
        cq = cm * q
        X, Y = v[lo], v[hi]
        S = _sum_no_wrap(X, Y, "inverse stage %d: X + Y" % beta)
        Xc = _sum_no_wrap(X, arr(cq), "inverse stage %d: X + cq" % beta)
        if bool((Xc < Y).any()):
            raise Wrapped("inverse stage %d: X + %dq - Y is negative" % (beta, cm))
        D = Xc - Y
        margin = int((Xc - Y).min()) / q
        peak = max(int(S.max()), int(Xc.max()))
        # twiddles: in the last round the butterflies whose index bits low5 .. beta-1 are zero take theirs times n^-1
        zh = ((lo >> low5) & ((1 << max(beta - low5, 0)) - 1)) == 0 if beta >= low5 else np.zeros(len(lo), bool)
        w = np.where(zh, tb.invn[0][ti], tb.inv[0][ti])
        wp = np.where(zh, tb.invn[1][ti], tb.inv[1][ti])
        red = (pol["inv_mask"] >> beta) & 1
        fin_red = last and not (near and not ex) and 2 * pol["cmul"][beta] > tq
        if red or fin_red:
            if ex and not near:
                if int(S.max()) >= 4 * q:
                    raise Wrapped("inverse stage %d: csub(S, 2q) on S >= 4q" % beta)
                Sr = w_csub(S, 2 * q)
            elif hl == 3 and not near:
                if int(S.max()) >= 8 * q:
                    raise Wrapped("inverse stage %d: csub(S, 4q) on S >= 8q" % beta)
                Sr = w_csub(S, 4 * q)
            else:
                Sr = w_reduce_sel(S, c, near)
        else:
            Sr = S
        if last:                                             # summed in every stage of the last round: the explicit n^-1
            zs = ((lo >> low5) & ((1 << (logn - 1 - low5)) - 1)) == 0
            ni, nip = U(tb.ninv), U(shoup(tb.ninv, q))
            Sn = w_mul_shoup2(S, ni, nip, q) if ex else w_mul_shoup4m(S, ni, nip, q)
            Sr = np.where(zs, Sn, Sr)
        Tm = w_mul_shoup2(D, w, wp, q) if ex else w_mul_shoup4m(D, w, wp, q)
        if int(Tm.max()) >= tq * q:
            raise Wrapped("inverse stage %d: product outside [0, %dq)" % (beta, tq))
        v[lo], v[hi] = Sr, Tm
        trace.add("inv%d" % beta, peak, margin, (M64 - peak) / q)
    return v


def model_canon_inverse(v, tb, hl, near):
    q = tb.q
    if hl > 2:
        if near:
            v = w_reduce_2q_near(v, tb.c)[1]
        else:
            if int(v.max()) >= 4 * q:
                raise Wrapped("canon_after_inverse: value >= 4q")
            v = w_csub(v, 2 * q)
    if int(v.max()) >= 2 * q:
        raise Wrapped("canon_after_inverse: value >= 2q in front of canon_2q")
    return w_csub(v, q)


def run_model(op, a, b, tb, hl, near):
    """op = 'fwd' | 'inv' | 'mul' (forward -> (.) b -> inverse; b: canonical words of bhat).  Returns (canonical result, Trace);
    raises Wrapped when an operation wraps 2^64, goes negative or leaves a promised range."""
    tr = Trace(tb.q)
    if op == "fwd":
        return model_canon_forward(model_forward(a, tb, hl, near, tr), tb, hl, near), tr
    if op == "inv":
        return model_canon_inverse(model_inverse(a, tb, hl, near, tr), tb, hl, near), tr
    f = model_forward(a, tb, hl, near, tr)
    m, lazy = model_fused_mul(f, b, tb, hl, near)
    return model_canon_inverse(model_inverse(m, tb, hl, near, tr, in2q=lazy), tb, hl, near), tr


# exact transforms in Python integers (what the model's canonical result must equal; also the back-solves of the stress inputs)
def exact_forward(a, tb):
    v, q, logn = [int(x) for x in a], tb.q, tb.logn
    for s in range(logn):
        bit = logn - 1 - s
        for i in range(tb.n):
            if not (i >> bit) & 1:
                j = i + (1 << bit)
                t = v[j] * tb.fw[(1 << s) + (i >> (logn - s))] % q
                v[i], v[j] = (v[i] + t) % q, (v[i] - t) % q
    return v


def exact_inverse(a, tb, stages=None, scale=True):
    v, q, logn = [int(x) for x in a], tb.q, tb.logn
    for beta in range(logn if stages is None else stages):
        for i in range(tb.n):
            if not (i >> beta) & 1:
                j = i + (1 << beta)
                x, y = v[i], v[j]
                v[i], v[j] = (x + y) % q, (x - y) * tb.iw[(1 << (logn - 1 - beta)) + (i >> (beta + 1))] % q
    return [x * tb.ninv % q for x in v] if scale else v


def undo_forward_stages(state, tb, upto):
    """the input whose exact forward transform has the canonical `state` in front of CT stage `upto` (stages 0 .. upto-1 inverted)"""
    v, q, logn = [int(x) for x in state], tb.q, tb.logn
    inv2 = (q + 1) // 2
    for s in range(upto - 1, -1, -1):
        bit = logn - 1 - s
        for i in range(tb.n):
            if not (i >> bit) & 1:
                j = i + (1 << bit)
                winv = tb.iw[(1 << s) + (i >> (logn - s))]          # (entry i of the two tables are inverses of each other)
                a_, b_ = v[i], v[j]                       # a = u + t, b = u - t
                u, t = (a_ + b_) * inv2 % q, (a_ - b_) * inv2 % q
                v[i], v[j] = u, t * winv % q
    return v


def undo_inverse_stages(state, tb, upto):
    """the input whose exact (unscaled) GS stages 0 .. upto-1 produce the canonical `state`"""
    v, q, logn = [int(x) for x in state], tb.q, tb.logn
    inv2 = (q + 1) // 2
    for beta in range(upto - 1, -1, -1):
        for i in range(tb.n):
            if not (i >> beta) & 1:
                j = i + (1 << beta)
                winv = tb.fw[(1 << (logn - 1 - beta)) + (i >> (beta + 1))]
                s_, d_ = v[i], v[j] * winv % q                 # s = x + y, d = x - y
                v[i], v[j] = (s_ + d_) * inv2 % q, (s_ - d_) * inv2 % q
    return v


# ---------------------------------------------------------------------------------------------------------------------------
# 3. interval checker of the policy
# ---------------------------------------------------------------------------------------------------------------------------
def check_policy(pol, hl, near, qmax, split16=False, fused=False):
    """Propagates bounds (multiples of q: a value is BELOW bound * q) through forward, the fused hand-over and inverse, using only
    what the primitives promise.  Returns the list of violations (empty: the policy is sound for every q <= qmax of the class)."""
    bad = []
    k = qmax.bit_length()
    tq, ex, logn = pol["tq"], hl <= 2, pol["logn"]
    assert tq == tq_of(hl)

    def fits(bound, what):
        if bound * qmax > (1 << 64):
            bad.append("%s: %d q can reach 2^64" % (what, bound))

    def reduce_domain(bound, what):
        # reduce_2q: B <= 66 or B q < 2^(k+5); reduce_2q_near: any 64-bit word
        fits(bound, what)
        if not near and not (bound <= 66 or bound * qmax < (1 << (k + 5))):
            bad.append("%s: %d q outside reduce_2q's domain" % (what, bound))
        return 2

    # ---- forward ----
    B = 1
    if split16:          # the stage that couples the two 2^15 halves: canonical U, V
        fits(1 + tq, "coupling forward U + Tm / U + cq - Tm")
        reduce_domain(1 + tq, "coupling forward reduce")
        B = 2            # the lower half enters the 2^15 rounds below 2q (the upper one is canonicalised for the store)
    peak_f = B
    for s in range(logn):
        Ub = B
        if (pol["fwd_mask"] >> s) & 1:
            Ub = reduce_domain(B, "forward stage %d reduce" % s)
        fits(B, "forward stage %d product operand" % s)               # any 64-bit word, but it must BE one
        # cq = TQ q against the product's promised range [0, TQ q)
        fits(Ub + tq, "forward stage %d U + T / U + cq" % s)
        B = Ub + tq
        peak_f = max(peak_f, B)
    reduce_domain(B, "canon_after_forward")
    # ---- hand-over ----
    inb, cm0 = 1, pol["cmul"][0]
    if fused and fused_is_lazy(hl, near):
        inb, cm0 = 2, 2      # reduce_2q_near (any word) -> mul_fold_near (x < 2q, b < q < 2^k) -> [0, 2q): IN2Q
    # ---- inverse ----
    B = inb
    peak_i = B
    for s in range(logn):
        last = s == logn - 1
        cm = cm0 if s == 0 else pol["cmul"][s]
        if cm < B:
            bad.append("inverse stage %d: cq = %d q below the bound %d q of what is subtracted" % (s, cm, B))
        fits(2 * B, "inverse stage %d X + Y" % s)
        fits(B + cm, "inverse stage %d X + cq" % s)
        peak_i = max(peak_i, 2 * B, B + cm)
        Sb = 2 * B
        red = (pol["inv_mask"] >> s) & 1
        fin_red = last and not (near and not ex) and 2 * pol["cmul"][s] > tq
        if red or fin_red:
            if ex and not near:
                if Sb > 4:
                    bad.append("inverse stage %d: csub(S, 2q) on a sum that can reach %d q" % (s, Sb))
                Sb = 2
            elif hl == 3 and not near:
                if Sb > 8:
                    bad.append("inverse stage %d: csub(S, 4q) on a sum that can reach %d q" % (s, Sb))
                Sb = 4
            else:
                Sb = reduce_domain(Sb, "inverse stage %d reduce" % s)
        B = max(Sb, tq)          # (the n^-1 products of the last stage are products too: below TQ q)
    if ex and B > 2:
        bad.append("canon_after_inverse: canon_2q on %d q" % B)
    if not ex and not near and B > 4:
        bad.append("canon_after_inverse: one subtraction of 2q on %d q" % B)
    if split16:              # canonical X, Y: canon_2q(X + Y), mul_shoup(X + q - Y), reduce, canon
        fits(2, "coupling inverse X + Y")
        reduce_domain(tq, "coupling inverse reduce")
    return bad, peak_f, peak_i


# ---------------------------------------------------------------------------------------------------------------------------
# probe files
# ---------------------------------------------------------------------------------------------------------------------------
def write_probe_input(path, records):
    """records: (op name, hl, near, consts, [arrays of Python ints]) -- per-tuple arrays first, then the per-workgroup W, WP"""
    words = [MAGIC, len(records)]
    for op, hl, near, c, arrays in records:
        count = len(arrays[0])
        words += [OP_ID[op], hl or 0, int(bool(near)), c["q"], c["k"], c["mu"], count, len(arrays)]
        for a in arrays:
            words.append(len(a))
            words += [int(x) for x in a]
    np.array(words, dtype=np.uint64).tofile(path)


def read_probe_output(path, records):
    out = np.fromfile(path, dtype=np.uint64)
    res, pos = [], 0
    for op, hl, near, c, arrays in records:
        count = len(arrays[0])
        if op == "mul_wide":
            lo, hi = out[pos:pos + count], out[pos + count:pos + 2 * count]
            res.append(list(zip((int(x) for x in lo), (int(x) for x in hi))))
            pos += 2 * count
        else:
            res.append([int(x) for x in out[pos:pos + count]])
            pos += count
    assert pos == len(out), (pos, len(out))
    return res
