#!/usr/bin/env python3
"""Whether two builds hold the same device code: the gfx950 code object of every unit of libhiprz.so and of the query, order and bake
units, unbundled the way tools/check_kernels.py does, compared byte for byte.  For a change that claims to touch host code only.

usage: tools/same_code_objects.py OTHER_CSRC     (a built rayzath_amd/csrc of another checkout; this checkout's is the other side)
Prints one line per unit with both sizes and exits 1 if any differs."""
import hashlib
import os
import subprocess
import sys
import tempfile

import check_kernels as ck

SATELLITES = ("query/hiprz_query.o", "order/hiprz_order.o", "bake/hiprz_bake.o")


def code_object(obj):
    """the bytes of the gfx950 code object in an object file (one bundle per unit); none for a unit that defines no kernel"""
    if ".hip_fatbin" not in ck.run(os.path.join(ck.LLVM, "llvm-readelf"), "-S", "-W", obj):
        return b""
    with tempfile.TemporaryDirectory() as tmp:
        fat, co = os.path.join(tmp, "fatbin"), os.path.join(tmp, "co")
        subprocess.run([os.path.join(ck.LLVM, "llvm-objcopy"), "--dump-section", f".hip_fatbin={fat}", obj, os.path.join(tmp, "discard")], check=True, capture_output=True)
        subprocess.run([os.path.join(ck.LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", f"--input={fat}", f"--targets={ck.TARGET}", f"--output={co}"],
                       check=True, capture_output=True)
        return open(co, "rb").read()


def main():
    other = sys.argv[1]
    units = sorted(f[:-4] + ".o" for f in os.listdir(ck.CSRC) if f.endswith(".hip")) + list(SATELLITES)
    differ = 0
    for unit in units:
        a, b = code_object(os.path.join(other, unit)), code_object(os.path.join(ck.CSRC, unit))
        same = a == b
        differ += not same
        print(f"{unit:34s} {len(a):9d} {len(b):9d} bytes  sha256 {hashlib.sha256(b).hexdigest()[:16]}  {'identical' if same else 'DIFFERENT'}")
    print(f"{len(units)} units, {differ} differ")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
