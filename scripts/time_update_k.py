"""Bulk trailing update against the depth K of one launch: the per-tile fixed cost (first loads, C read-modify-write, dispatch)
against the K-proportional MFMA loop.
  time_update_k.py [M ...]                                  one variant (VARIANT, default 0), 5 launches per figure
  time_update_k.py --variants 31,30 --pairs 5 --reps 170 M  the variants ALTERNATED in one process, `pairs` times each,
                                                            `reps` launches per figure (short measurements of this kernel
                                                            read low), then the median of each and the ratio per pair
Variants (csrc/gemm.hip, launch_trailing_update_as): 0 the fit's launch, 3 the fp32-product kernel of the mixed fit,
30 / 31 whole 128 x 128 tiles only on the ring loop / on the register-staged loop."""
import argparse
import ctypes as C, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import albatross_amd as ab
from albatross_amd import _capi as capi

ap = argparse.ArgumentParser()
ap.add_argument("M", nargs="*", type=int, default=[15872, 8192])
ap.add_argument("--variants", default=os.environ.get("VARIANT", "0"))
ap.add_argument("--pairs", type=int, default=1)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--ks", default="128,256,512,768,1024,1536,2048")
args = ap.parse_args()
variants = [int(v) for v in args.variants.split(",")]
ks = [int(k) for k in args.ks.split(",")]

ctx = ab.Context(0)
lib = capi.load_debug()
lib.agp_debug_time_trailing_update.restype = C.c_int
lib.agp_debug_time_trailing_update.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_int, C.POINTER(C.c_double)]
for M in args.M:
    tiles = (M // 128) * (M // 128 + 1) // 2
    for K in ks:
        flop = 2.0 * K * 128 * 128 * tiles
        seen = {v: [] for v in variants}
        for pair in range(args.pairs):
            for v in variants:
                ms = C.c_double()
                st = lib.agp_debug_time_trailing_update(ctx._h, M, K, v, args.reps, C.byref(ms))
                if st != 0:
                    sys.exit(f"agp_debug_time_trailing_update: status {st} (M={M} K={K} variant={v})")
                seen[v].append(ms.value)
                print(f"M={M:6d} K={K:5d} variant {v:2d} run {pair}: {ms.value:8.3f} ms  {flop / ms.value / 1e9:6.1f} TF   "
                      f"{ms.value * 1e3 / (tiles / 512.0):7.1f} us per round of 512 tiles", flush=True)
        if args.pairs > 1 or len(variants) > 1:
            med = {v: statistics.median(seen[v]) for v in variants}
            line = "  ".join(f"variant {v}: median {med[v]:.3f} ms {flop / med[v] / 1e9:.1f} TF" for v in variants)
            if len(variants) == 2:
                a, b = variants
                ratios = [y / x for x, y in zip(seen[a], seen[b])]
                line += f"  | time {b} / time {a} per pair: " + " ".join(f"{r:.4f}" for r in ratios)
            print(f"M={M:6d} K={K:5d} {line}", flush=True)
