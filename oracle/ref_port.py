"""Port recipe for the reference tree (test infrastructure): writes translated copies under oracle/_ref/src.

    python ref_port.py REFERENCE_ROOT OUT_DIR [HIPIFY]

Nothing of the reference is stored in this repository; this script finds its places by file name, pattern and
function name only.  Steps, all mechanical:
  1. run hipify-perl over the ten BFV_Scheme headers, BFV_Scheme/decryption_test.cu and old/ntt_30bit.cuh
     (the latter into OUT_DIR/ref30/: its function names collide with the 60-bit header's);
  2. close the launch brackets the reference writes with a space inside (hipcc does not accept the spaced form);
  3. drop the include lines the translation emptied;
  4. in uint128.h, cut from the definition of sub128 (the first of the two inline-PTX functions, which are the
     last two of the file) to the end, and include ref_shim.h there;
  5. in uint128.h, route the shifts of the low / high words by `shift` and `64 - shift` through ref_shift.h: PTX
     clamps a shift count of 64 or more to a zero result and the reference's 62-bit Barrett relies on it, gfx950
     takes the count modulo 64 (ref_shift.h has the whole story).
"""
import glob
import os
import re
import subprocess
import sys


def translate(hipify, src):
    text = subprocess.run([hipify, src], check=True, stdout=subprocess.PIPE).stdout.decode("utf-8", "replace")
    text = re.sub(r"<<\s+<", "<<<", text)
    text = re.sub(r">>\s+>", ">>>", text)
    text = re.sub(r'^[ \t]*#include[ \t]*""[ \t]*\r?\n', "", text, flags=re.M)
    return text


def cut_ptx(text):
    """uint128.h: everything from the line that opens the definition of sub128 goes; the shim comes in."""
    m = re.search(r"^[^\n]*\bvoid\s+sub128\s*\(", text, flags=re.M)
    if m is None or "mul64" not in text[m.start():] or "asm" not in text[m.start():]:
        raise SystemExit("ref_port: uint128.h does not end with the sub128 / mul64 PTX pair; the recipe needs a look")
    if "asm" in text[:m.start()]:
        raise SystemExit("ref_port: inline assembly before sub128 in uint128.h; the recipe needs a look")
    return text[:m.start()] + '#include "ref_shim.h"\n'


SHIFT = re.compile(r"((?:\b\w+\.)?\b(?:low|high))\s*(<<|>>)\s*(shift\b|\(64 - shift\))")


def clamp_shifts(text):
    """uint128.h: WORD << shift, WORD >> shift, WORD << (64 - shift), WORD >> (64 - shift) on the 64-bit members only"""
    text, count = SHIFT.subn(lambda m: "%s(%s, %s)" % ("ref_shl64" if m.group(2) == "<<" else "ref_shr64", m.group(1), m.group(3)), text)
    if count != 12:
        raise SystemExit("ref_port: expected 12 word shifts in uint128.h's shift members, found %d; the recipe needs a look" % count)
    first = re.search(r"^[ \t]*class\s+uint128_t\b", text, flags=re.M)
    if first is None:
        raise SystemExit("ref_port: uint128.h has no class uint128_t")
    return text[:first.start()] + '#include "ref_shift.h"\n' + text[first.start():]


def main(argv):
    ref, out = argv[1], argv[2]
    hipify = argv[3] if len(argv) > 3 else "hipify-perl"
    bfv = os.path.join(ref, "BFV_Scheme")
    headers = sorted(glob.glob(os.path.join(bfv, "*.cuh")) + glob.glob(os.path.join(bfv, "*.h")))
    if len(headers) != 10:
        raise SystemExit("ref_port: expected the ten BFV_Scheme headers under %s, found %d" % (bfv, len(headers)))
    jobs = [(h, os.path.join(out, os.path.basename(h))) for h in headers]
    jobs.append((os.path.join(bfv, "decryption_test.cu"), os.path.join(out, "decryption_test.hip")))
    jobs.append((os.path.join(ref, "old", "ntt_30bit.cuh"), os.path.join(out, "ref30", "ntt_30bit.cuh")))
    for src, dst in jobs:
        text = translate(hipify, src)
        if os.path.basename(src) == "uint128.h":
            text = clamp_shifts(cut_ptx(text))
        if re.search(r"\basm\b", text):
            raise SystemExit("ref_port: inline assembly left in %s" % src)
        os.makedirs(os.path.dirname(dst), exist_ok=True)
        with open(dst, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
