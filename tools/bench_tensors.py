#!/usr/bin/env python
"""The tensor path against the raw device-resident loop, one engine, 1024 streams x 1024
detections (bench.py's frames: bench.stage_frames), a 40-frame pre-roll and 20 timed frames.

  (a) raw: yta_bytetrack_update_device, the loop bench.py times (frames and offsets staged in HBM,
      S * track_capacity unpacked rows left in HBM);
  (b) ByteTrackEngine.update_tensors with float64 input (read in place) and with float32 input
      (widened by the ingest kernel), packed rows / offsets / row_stream tensors out.

Every leg has an engine of its own, created with bench.py's parameters, and ends with a wait for
the device inside the timed region.  One JSON line per leg, then a summary line with (b) / (a).
--repo DIR imports the package and bench.py from another checkout (the parent commit's build, which
has no update_tensors: only (a) runs there).

    python tools/bench_tensors.py [--out profiles/tensors/NAME.jsonl]
"""
import argparse
import ctypes
import json
import os
import sys
import time


def parse():
    p = argparse.ArgumentParser()
    p.add_argument("--streams", type=int, default=1024)
    p.add_argument("--n", type=int, default=1024)
    p.add_argument("--preroll", type=int, default=40)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--repeats", type=int, default=3, help="runs of every leg (fresh engine each)")
    p.add_argument("--cap-mult", type=int, nargs="+", default=[2],
                   help="track_capacity / n of the engines (bench.py: 2)")
    p.add_argument("--seed", type=int, default=1000)
    p.add_argument("--repo", default=None, help="import the package and bench.py from this tree")
    p.add_argument("--out", default=None, help="also append the JSON lines to this file")
    return p.parse_args()


def main():
    a = parse()
    repo = os.path.abspath(a.repo or os.path.join(os.path.dirname(__file__), ".."))
    sys.path.insert(0, repo)
    import torch

    import bench
    from yolo_tracking_amd import ByteTrackEngine, _lib

    S, N, PRE, K = a.streams, a.n, a.preroll, a.steps
    F = PRE + K
    d_dets, d_off = bench.stage_frames(N, F, bench.stream_seeds(a.seed, 0, S), 1, "cuda")
    d64, d_off = d_dets[0], d_off[0]          # [F][S*N][6] float64, [F][S+1] int32
    counts = [N] * S
    lines = []

    def emit(rec):
        rec = dict(rec, streams=S, n=N, preroll=PRE, steps=K, repo=os.path.basename(repo))
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    def engine(cm):
        return ByteTrackEngine(S, track_thresh=0.5, match_thresh=0.8, track_buffer=30,
                               frame_rate=30, device=0, track_capacity=cm * N, max_dets=N)

    def timed(step, eng):
        torch.cuda.synchronize()
        for f in range(PRE):
            step(f)
        torch.cuda.synchronize()
        _lib.check(eng.lib.yta_bytetrack_sync(eng.handle))
        t0 = time.perf_counter()
        for f in range(PRE, F):
            step(f)
        torch.cuda.synchronize()
        _lib.check(eng.lib.yta_bytetrack_sync(eng.handle))
        return time.perf_counter() - t0

    def raw_leg(cm):
        eng = engine(cm)
        cap, _ = eng.capacity()
        d_out = torch.empty((S * cap, 8), dtype=torch.float64, device="cuda")
        d_cnt = torch.zeros(S, dtype=torch.int32, device="cuda")
        fb, ob = S * N * 48, (S + 1) * 4

        def step(f):
            _lib.check(eng.lib.yta_bytetrack_update_device(
                eng.handle, ctypes.c_void_p(d64.data_ptr() + f * fb),
                ctypes.c_void_p(d_off.data_ptr() + f * ob), ctypes.c_void_p(d_out.data_ptr()),
                ctypes.c_void_p(d_cnt.data_ptr())))

        el = timed(step, eng)
        rows = int(d_cnt.sum())
        eng.close()
        return el, dict(out_rows_last=rows)

    def tensor_leg(cm, src):
        eng = engine(cm)
        keep = [None]

        def step(f):
            keep[0] = eng.update_tensors(src[f], counts=counts)

        el = timed(step, eng)
        st = eng.tensor_stats()
        rows = int(keep[0][1][-1])
        eng.close()
        return el, dict(out_rows_last=rows, **st)

    legs = [("raw_update_device", raw_leg, None)]
    if hasattr(ByteTrackEngine, "update_tensors"):
        d32 = d64.float()
        legs += [("update_tensors_f64", tensor_leg, d64), ("update_tensors_f32", tensor_leg, d32)]
    best = {}
    for cm in a.cap_mult:
        for r in range(a.repeats):
            for name, fn, src in legs:
                el, extra = fn(cm) if src is None else fn(cm, src)
                rate = S * K / el
                emit(dict(leg=name, cap_mult=cm, repeat=r, calls_per_s=rate,
                          ms_per_frame=1e3 * el / K, **extra))
                best[(name, cm)] = max(best.get((name, cm), 0.0), rate)
    for cm in a.cap_mult:
        base = best[("raw_update_device", cm)]
        emit(dict(leg="summary", cap_mult=cm,
                  best_calls_per_s={n: best[(n, c)] for (n, c) in best if c == cm},
                  ratio_to_raw={n: best[(n, c)] / base for (n, c) in best if c == cm}))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            for rec in lines:
                fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
