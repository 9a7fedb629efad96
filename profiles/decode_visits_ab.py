"""Same-process A/B of the visits of the grouped fused decode (kernels_rectdma.hip, VISITS): bench.py's default workload (8 distinct
4096x3000 stereo frames on the stereo head verged by 0.2 rad, slr_reconstruct_mf_batch) with SLR_OPT_DEBUG_FLAGS 0 (the default
frames per visit) and bit 10 (one frame per visit) in alternation.  Prints one JSON line per leg and a summary line: the library
profiler's slr_mf_rectify_decode_pair and slr_mf_match_triangulate us per frame, wall ms per frame, and whether both settings give
the same cloud checksums.  --legs 0 (or 1024) runs one setting only: for rocprofv3 runs, and for a library that predates bit 10.

    python3 profiles/decode_visits_ab.py [--rounds 4] [--batches 20] [--legs 0,1024] [--lib path/to/libslr_hip.so]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--lib", default=None, help="another build of libslr_hip.so (experiments)")
    ap.add_argument("--legs", default="0,1024", help="SLR_OPT_DEBUG_FLAGS of the legs of a round (alternating order)")
    ap.add_argument("--x87", type=int, default=0)
    ap.add_argument("--width", type=int, default=4096)
    ap.add_argument("--height", type=int, default=3000)
    args = ap.parse_args()
    import importlib
    import torch
    capi = importlib.import_module("structure-light-reconstructor_amd.capi")
    if args.lib:
        capi.LIB_PATH = os.path.abspath(args.lib)
    slr = importlib.import_module("structure-light-reconstructor_amd")
    synth = importlib.import_module("structure-light-reconstructor_amd.synth")
    W, H, F, BLACK = args.width, args.height, 8, 40
    dev = torch.device("cuda", 0)
    ctx = slr.Context(0)
    if args.x87:
        ctx.set_option(capi.OPT_EVAL_MODEL, 1)
    rig = synth.make_verged_rig(W, H, 0.2, -0.15)
    ctx.set_calibration(rig["calib"])
    synth.install_verged_maps(ctx, rig, W, H)
    stack = torch.stack([synth.render_mf_stack(W, H, seed=1000 + f, noise=2, device=dev) for f in range(F)])
    xyz = torch.empty((F, H, W, 3), dtype=torch.float32, device=dev)
    has = torch.empty((F, H, W), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    ctx.set_option(capi.OPT_PROFILE_STRIDE, 1)
    legs = [int(v) for v in args.legs.split(",")]
    res = {f: [] for f in legs}
    sums = {}
    for r in range(args.rounds):
        for flags in (legs if r % 2 == 0 else legs[::-1]):
            ctx.set_option(capi.OPT_DEBUG_FLAGS, flags)
            for _ in range(args.warmup):
                ctx.reconstruct_mf_batch(stack, BLACK, True, xyz=xyz, has=has)
            ctx.synchronize()
            ctx.profile_enable(True)
            ctx.profile_reset()
            t0 = time.perf_counter()
            for _ in range(args.batches):
                ctx.reconstruct_mf_batch(stack, BLACK, True, xyz=xyz, has=has)
            ctx.synchronize()
            wall = time.perf_counter() - t0
            pr = ctx.profile()
            ctx.profile_enable(False)
            leg = {"round": r, "debug_flags": flags, "wall_ms_per_frame": round(wall / (args.batches * F) * 1e3, 4)}
            for kn, short in (("slr_mf_rectify_decode_pair", "decode_us_per_frame"), ("slr_mf_match_triangulate", "match_us_per_frame")):
                if kn in pr and pr[kn][1]:
                    leg[short] = round(pr[kn][0] / pr[kn][1] * 1e3, 2)
            sums.setdefault(flags, set()).add(tuple(int(v) for v in ctx.cloud_checksums(xyz, has)))
            res[flags].append(leg)
            print(json.dumps(leg), flush=True)
    ctx.set_option(capi.OPT_DEBUG_FLAGS, 0)
    summ = {"lib": args.lib or "in-tree", "x87": args.x87, "rounds": args.rounds, "batches_per_leg": args.batches,
            "same_clouds": all(sums[f] == sums[legs[0]] for f in legs) and len(sums[legs[0]]) == 1}
    for flags, entries in res.items():
        for k in ("decode_us_per_frame", "match_us_per_frame", "wall_ms_per_frame"):
            v = sorted(e[k] for e in entries if k in e)
            if v:
                summ["flags_%d_%s" % (flags, k)] = {"min": v[0], "median": v[len(v) // 2], "max": v[-1]}
    a, b = summ.get("flags_%d_decode_us_per_frame" % legs[0]), summ.get("flags_%d_decode_us_per_frame" % legs[-1])
    if a and b and len(legs) == 2:
        summ["decode_gain_median"] = round(1.0 - a["median"] / b["median"], 4)
    summ["checksums"] = ["%016x" % (v & 0xFFFFFFFFFFFFFFFF) for v in sorted(sums[legs[0]])[0]]
    print(json.dumps(summ), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
