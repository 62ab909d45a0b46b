"""Python side of the reference harnesses (oracle/_ref/ref60, ref30): writes requests, reads responses.

TEST INFRASTRUCTURE ONLY.  The binaries are the reference's own kernels built for gfx950 by `make -C oracle ref`
(ref_port.py, ref_harness60.hip, ref_harness30.hip); the file format is documented in ref_proto.h.  A run is one
fresh child process under its own time limit; a non-zero exit status raises, and nothing is ever retried.
"""
import os
import subprocess
import tempfile

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
REF_DIR = os.path.join(_HERE, "_ref")
REF60 = os.path.join(REF_DIR, "ref60")
REF30 = os.path.join(REF_DIR, "ref30")
DECRYPTION_TEST = os.path.join(REF_DIR, "decryption_test")
BINARIES = (REF60, REF30, DECRYPTION_TEST)
RECIPE = tuple(os.path.join(_HERE, f) for f in ("Makefile", "ref_port.py", "ref_shim.h", "ref_shift.h", "ref_proto.h",
                                                "ref_harness60.hip", "ref_harness30.hip"))
SKIP_REASON = "oracle/_ref not built: no reference tree at build time"

REQ_MAGIC = 0x3151455246455221
RSP_MAGIC = 0x3150535246455221

# op codes of ref_harness60.hip (ref_harness30.hip shares 2, 3 and 7)
SELFCHECK_MUL64, SELFCHECK_SUB128 = 0, 1
FORWARD, INVERSE, FORWARD_DOUBLE, FORWARD_BATCH, INVERSE_BATCH = 2, 3, 4, 5, 6
BARRETT, BARRETT_BATCH, BARRETT_BATCH_3PARAM, BARRETT_INT = 7, 8, 9, 10
HALF_POLY_MUL, FULL_POLY_MUL = 11, 12
POLY_ADD, POLY_SUB, POLY_NEGATE, POLY_ADD_INTEGER, POLY_MUL_INT_T = 13, 14, 15, 16, 17
GENERATE_RANDOM_DEFAULT, GENERATE_RANDOM = 18, 19
TERNARY_XQ, UNIFORM_XQ, GAUSSIAN_XQ, CONVERT_TERNARY_GAUSSIAN_X2 = 20, 21, 22, 23
BFV_DRIVERS = 24
SELFCHECK_SHIFT = 25


def available():
    return all(os.access(b, os.X_OK) for b in BINARIES)


def reference_tree():
    """the reference checkout the recipe would use ($REFERENCE, else the Makefile's default), or None"""
    root = os.environ.get("REFERENCE")
    if not root:
        with open(os.path.join(_HERE, "Makefile")) as f:
            for line in f:
                if line.startswith("REFERENCE"):
                    root = line.split("=", 1)[1].strip()
                    break
    return root if root and os.path.isdir(os.path.join(root, "BFV_Scheme")) else None


def bit_length(q):
    """the reference's log2((double)q) + 1 (decryption_test.cu:69); equal to int.bit_length for every modulus used here"""
    return int(q).bit_length()


def modulus(q, psi=0, bits=None):
    """(q, mu, qbit, psi) with mu = floor(2^(2 qbit) / q) as the reference's programs derive it"""
    k = bit_length(q) if bits is None else int(bits)
    return (int(q), (1 << (2 * k)) // int(q), k, int(psi))


def pack_bytes(b):
    """bytes / uint8 array -> u64 words, zero padded"""
    b = np.frombuffer(bytes(b), dtype=np.uint8) if not isinstance(b, np.ndarray) else np.ascontiguousarray(b, dtype=np.uint8)
    pad = (-b.size) % 8
    if pad:
        b = np.concatenate([b, np.zeros(pad, dtype=np.uint8)])
    return b.view("<u8").astype(np.uint64)


def pack_u32(a):
    return pack_bytes(np.ascontiguousarray(a, dtype="<u4").view(np.uint8))


def unpack_u32(w):
    return np.ascontiguousarray(w, dtype="<u8").view("<u4").astype(np.uint32)


def unpack_bytes(w):
    return np.ascontiguousarray(w, dtype="<u8").view(np.uint8)


class Case:
    def __init__(self, op, n, moduli=(), args=(), words=()):
        self.op, self.n = int(op), int(n)
        self.moduli = [tuple(int(x) for x in m) for m in moduli]
        self.args = [int(x) for x in args]
        parts = [np.ascontiguousarray(w, dtype=np.uint64).reshape(-1) for w in (words if isinstance(words, (list, tuple)) else [words])]
        self.words = np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint64)

    def encode(self):
        head = [self.op, self.n, len(self.moduli), len(self.args), self.words.size]
        flat = head + [x for m in self.moduli for x in m] + self.args
        return np.concatenate([np.array(flat, dtype=np.uint64), self.words])


def encode_request(cases):
    return np.concatenate([np.array([REQ_MAGIC, len(cases)], dtype=np.uint64)] + [c.encode() for c in cases]).astype("<u8").tobytes()


def decode_response(blob, ncases):
    w = np.frombuffer(blob, dtype="<u8").astype(np.uint64)
    assert w.size >= 2 and int(w[0]) == RSP_MAGIC and int(w[1]) == ncases, "malformed response"
    out, at = [], 2
    for _ in range(ncases):
        nw = int(w[at])
        out.append(w[at + 1:at + 1 + nw].copy())
        at += 1 + nw
    assert at == w.size, "trailing words in response"
    return out


# The reference orders some kernels across streams by nothing but timing: decryption_rns launches its rounding kernel on one stream
# while the kernel that writes its input runs on another (bfv_decryption.cuh:133-137), and full_poly_mul_device multiplies on stream2
# what stream1 is still transforming (poly_arithmetic.cuh:298-300).  On an MI355X decryption_test loses that race and prints
# `Computations are wrong.`; with every kernel launch serialized -- the HIP runtime's AMD_SERIALIZE_KERNEL=3, the counterpart of
# CUDA_LAUNCH_BLOCKING -- the launch order of the source is the execution order and it prints `Computations are correct.`.  The
# reference binaries are therefore always run that way; nothing else in this project reads the variable.
CHILD_ENV = {"AMD_SERIALIZE_KERNEL": "3"}


def run(binary, cases, timeout=120, env=None):
    """one fresh child process for the whole request; returns the output words per case.  env: additions to the child's environment
    (on top of CHILD_ENV)"""
    env = dict(CHILD_ENV, **(env or {}))
    with tempfile.TemporaryDirectory() as d:
        req, rsp = os.path.join(d, "request.bin"), os.path.join(d, "response.bin")
        with open(req, "wb") as f:
            f.write(encode_request(cases))
        p = subprocess.run([binary, req, rsp], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=timeout,
                           env=dict(os.environ, **env) if env else None)
        if p.returncode != 0:
            raise RuntimeError("%s exited with status %d: %s" % (os.path.basename(binary), p.returncode, p.stdout.decode("utf-8", "replace")[-2000:]))
        with open(rsp, "rb") as f:
            return decode_response(f.read(), len(cases))
