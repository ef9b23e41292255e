#!/usr/bin/env python3
"""Route table of a libinsr_hip.so: every host-side routing answer of the backward paths, one line per
query and argument tuple, through the public C ABI only (include/insr_siren.h) -- so the same script
runs against any build of the library, and two builds route alike iff their tables are byte-identical.

    python tools/route_table.py [--lib PATH] > table.txt

Without a GPU the library answers for 256 CUs and no occupancy; on one, the occupancy branches of the
launch shapes get real values.  ("Backward routing".)
"""
import argparse
import ctypes
import os
import sys

try:
    import torch  # noqa: F401  (first, so the library binds to the HIP runtime torch loads)
except ImportError:
    pass

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VALUE, GRAD, LAP = 0, 1, 2
BPREC_SHIFT, POLICY_SHIFT, F16_SHIFT, TILES_SHIFT, WIDE128 = 12, 16, 19, 23, 1 << 9
SHAPES = [(2, 1, 4, 128), (2, 2, 4, 128), (2, 1, 5, 128), (2, 2, 5, 128), (1, 1, 4, 128), (3, 3, 4, 128),
          (2, 1, 3, 128), (2, 1, 0, 128), (2, 2, 4, 64), (1, 1, 3, 32), (3, 3, 5, 256), (2, 2, 0, 256)]
NS = [0, 1, 16, 17, 4095, 4096, 8191, 8192, 8355, 16708, 24575, 24576, 32767, 32768, 33092, 49151, 49152, 66844,
      131072]
_TCODE = {0: 0, 1: 1, 2: 2, 4: 3}
_MINB = {256: 0, 512: 1, 128: 2, 1024: 3}


def tiles_bits(fwd, bwd, min_blocks):
    return (_TCODE[fwd] | (_TCODE[bwd] << 2) | (_MINB[min_blocks] << 4)) << TILES_SHIFT


def knob_sets():
    """(label, mode bits): the full cross of policy x fp16 mask x WIDE128, then at policy 0 each backward
    precision and the two tile knobs, then the two malformed codes."""
    out = []
    for pol in range(6):
        for f16 in (None, 0, 3, 4, 7):
            for wide in (0, 1):
                bits = ((pol + 1) << POLICY_SHIFT) | (0 if f16 is None else (f16 + 1) << F16_SHIFT) | (WIDE128 * wide)
                out.append(("p%d,f%s,w%d" % (pol, "d" if f16 is None else f16, wide), bits))
    for prec in range(5):  # f32, bf16x6, bf16x3, bf16, f16x3
        out.append(("bprec%d" % prec, (prec + 1) << BPREC_SHIFT))
    out.append(("tiles1,4,512", tiles_bits(1, 4, 512)))
    out.append(("tiles0,0,128", tiles_bits(0, 0, 128)))
    out.append(("badpolicy", 7 << POLICY_SHIFT))
    out.append(("badf16", 9 << F16_SHIFT))
    return out


def load(path):
    lib = ctypes.CDLL(path)
    I, L = ctypes.c_int, ctypes.c_long
    sig = {
        "insr_jet_bwd_path": (I, [L, I, I, I, I, I]),
        "insr_jet_bwd_kernel": (I, [L, I, I, I, I, I]),
        "insr_jet_bwd_is_wide": (I, [L, I, I, I]),
        "insr_jet_bwd_work_bytes": (L, [L, I, I, I, I, I]),
        "insr_jet_partial_blocks": (I, [L, I, I, I]),
        "insr_jet_partial_bytes": (L, [L, I, I, I, I, I]),
        "insr_jet_split_tiles": (I, [L, I, I, I, I]),
        "insr_jet_bwd_seed_rows": (I, [L, I, I, I, I, I]),
        "insr_jet_wide_launch_threads": (I, [L, I, I, I, I, I, ctypes.POINTER(L)]),
        "insr_jet_bwd_multi_work_bytes": (L, [ctypes.POINTER(L), I, I, I, I, I, I]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--lib", default=os.path.join(ROOT, "insr-pde_amd", "lib", "libinsr_hip.so"))
    a = ap.parse_args()
    lib = load(a.lib)
    w = sys.stdout.write
    t3 = (ctypes.c_long * 3)()
    for din, dout, L, W in SHAPES:
        for jm in (VALUE, GRAD, LAP):
            for label, bits in knob_sets():
                mode = jm | bits
                for n in NS:
                    key = "%d,%d,%d,%d m%d %s n%d" % (din, dout, L, W, jm, label, n)
                    full = (n, din, dout, L, W, mode)
                    w("path %s %d\n" % (key, lib.insr_jet_bwd_path(*full)))
                    w("kernel %s %d\n" % (key, lib.insr_jet_bwd_kernel(*full)))
                    w("is_wide %s %d\n" % (key, lib.insr_jet_bwd_is_wide(n, din, W, mode)))
                    w("work_bytes %s %d\n" % (key, lib.insr_jet_bwd_work_bytes(*full)))
                    w("partial_blocks %s %d\n" % (key, lib.insr_jet_partial_blocks(n, din, W, mode)))
                    w("partial_bytes %s %d\n" % (key, lib.insr_jet_partial_bytes(*full)))
                    w("split_tiles_fwd %s %d\n" % (key, lib.insr_jet_split_tiles(n, din, W, mode, 0)))
                    w("split_tiles_bwd %s %d\n" % (key, lib.insr_jet_split_tiles(n, din, W, mode, 1)))
                    w("seed_rows %s %d\n" % (key, lib.insr_jet_bwd_seed_rows(*full)))
                    t3[0] = t3[1] = t3[2] = -7
                    rc = lib.insr_jet_wide_launch_threads(n, din, dout, L, W, mode, t3)
                    w("wide_threads %s %d %d %d %d\n" % (key, rc, t3[0], t3[1], t3[2]))
                    for jobs in ([n], [n, 162, 162], [162, 0, 162]):
                        arr = (ctypes.c_long * len(jobs))(*jobs)
                        wb = lib.insr_jet_bwd_multi_work_bytes(arr, len(jobs), din, dout, L, W, mode)
                        w("multi_work_bytes %s %s %d\n" % (key, "+".join(map(str, jobs)), wb))


if __name__ == "__main__":
    main()
