"""LMBN-n's pooling stage and neck alone on the MI355X (appearance/lmbn.py, csrc/lmbn.hip): three
random (N, 512, 16, 8) maps, as the branches leave them at 256 x 128 crops, through
yta_lmbn_pool (three launches, each map read once) and through the neck both ways: one
yta_lmbn_neck launch (fused) and seven yta_osnet_pointwise launches plus the channel heads' affine
(unfused).  Times are CUDA-event averages over --reps back-to-back calls after a warm-up, so they
include what a launch costs on the stream; the pool's bandwidth is the three maps' bytes over its
time.  Under `rocprofv3 --kernel-trace --stats` the same run gives the kernels' own times.
Prints JSON lines."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--crops", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    import torch
    from yolo_tracking_amd.appearance.lmbn import LMBNReID, random_state_dict
    sd = random_state_dict(0, randomise_bn=True)
    n = args.crops

    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return 1000 * e0.elapsed_time(e1) / args.reps        # microseconds

    for half in (False, True):
        nets = {f: LMBNReID("lmbn_n", sd, device="cuda:0", half=half, fused_neck=f)
                for f in (True, False)}
        g = torch.Generator(device="cuda").manual_seed(1)
        maps = [torch.randn((n, 512, 16, 8), generator=g, device="cuda", dtype=nets[True].dtype)
                for _ in range(3)]
        pool_us = timed(lambda: nets[True]._pool_hip(*maps))
        nbytes = sum(m.numel() * m.element_size() for m in maps)
        v, mc = nets[True]._pool_hip(*maps)
        neck = {f: timed(lambda f=f: nets[f]._neck_hip(v, mc)) for f in (True, False)}
        same = torch.equal(nets[True]._neck_hip(v, mc), nets[False]._neck_hip(v, mc))
        dt = "f16" if half else "f32"
        print(json.dumps({"metric": "LMBN pool", "crops": n, "dtype": dt, "launches": 3,
                          "bytes_read": nbytes, "us": pool_us,
                          "read_TB_per_s": nbytes / (pool_us * 1e-6) / 1e12}))
        print(json.dumps({"metric": "LMBN neck", "crops": n, "dtype": dt,
                          "fused_us": neck[True], "unfused_us": neck[False],
                          "unfused_over_fused": neck[False] / neck[True],
                          "equal_bits": bool(same)}))


if __name__ == "__main__":
    main()
