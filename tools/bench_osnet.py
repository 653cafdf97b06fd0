"""ReID producer end to end on the MI355X: crops of S camera streams x M
detections (1920x1080 BGR, one yta_reid_preprocess_device launch) + the OSNet forward
(appearance/osnet.py: folded BatchNorms, channels-last, batched branches; random weights of the
named variant, any key of appearance/osnet.py VARIANTS: the plain widths, osnet_ibn_* and
osnet_ain_* with their instance norms) + global normalisation, features left on the device.  Reports crops/s for the
network alone and for the whole get_features path, float32 and float16.  Prints JSON lines.
--variant mobilenetv2_x1_0 / mobilenetv2_x1_4 (appearance/mobilenetv2.py) runs the same measurement
on MobileNetV2: the HIP forward with the fused expand + depthwise kernel ("fused": true), with the
two layers as two launches ("fused": false), and the same folded graph on PyTorch's kernels in
NHWC and NCHW ("hip_blocks": false), the baseline a model=<torch module> user gets.
--variant mlfn (appearance/mlfn.py) measures the MLFN HIP forward against the same folded graph on
PyTorch's kernels (hip=False, "hip_blocks": false) on the same device, float32 and float16.
--variant clip (appearance/clip.py) does the same for the CLIP-ReID ViT-B/16, in chunks of
appearance.clip.CHUNK crops.
--variant lmbn_n (appearance/lmbn.py) measures the LMBN-n HIP forward with the fused neck (one
yta_lmbn_neck launch, "fused": true), with the unfused neck (seven yta_osnet_pointwise launches
and the channel heads' affine, "fused": false), and the folded graph on PyTorch's kernels
("hip_blocks": false), float32 and float16."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    from yolo_tracking_amd.appearance.reid_multibackend import FAMILIES
    ap.add_argument("--variant", default="osnet_x0_25",
                    choices=[v for family, _ in FAMILIES for v in sorted(family.VARIANTS)],
                    help="OSNet variant (plain, osnet_ibn_* or osnet_ain_*; default osnet_x0_25) "
                         "or mobilenetv2_x1_0 / mobilenetv2_x1_4, or mlfn, or lmbn_n, or clip")
    ap.add_argument("--crops", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=10)
    args = ap.parse_args()
    import torch
    from yolo_tracking_amd.appearance import ReIDDetectMultiBackend
    from yolo_tracking_amd.appearance.clip import CHUNK as CLIP_CHUNK
    family, cls = next(f for f in FAMILIES if args.variant in f[0].VARIANTS)
    kind = family.__name__.rsplit(".", 1)[1]   # osnet, mobilenetv2, mlfn, lmbn or clip
    rng = np.random.default_rng(0)
    H, W, n = 1080, 1920, args.crops
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    wh = rng.uniform(48, 192, (n, 2))
    xy = rng.uniform(0, 1, (n, 2)) * [W - 200, H - 200]
    boxes = np.concatenate([xy, xy + wh], 1)
    # per family: the metric's label and one (half, chunk, hip, channels_last, fused) per run
    if kind == "clip":   # the HIP forward and the folded graph on PyTorch's kernels, its own chunk
        label = "CLIP-ReID"
        configs = [(half, CLIP_CHUNK, hip, False, None) for half in (False, True)
                   for hip in (True, False)]
    elif kind == "mlfn":   # the HIP forward and the folded graph on PyTorch's kernels, NCHW
        label = "MLFN"
        configs = [(half, 1024, hip, False, None) for half in (False, True) for hip in (True, False)]
    elif kind == "lmbn":   # the fused and the unfused neck, and the graph on PyTorch's kernels
        label = "LMBN"
        configs = [(half, 1024, hip, not hip, fused) for half in (False, True)
                   for hip, fused in ((True, True), (True, False), (False, None))]
    elif kind == "mobilenetv2":
        label = "MobileNetV2"
        configs = [(half, 1024, hip, cl, fused) for half in (False, True)
                   for hip, cl, fused in ((True, False, True), (True, False, False),
                                          (False, True, None), (False, False, None))]
    else:
        label = "OSNet"
        configs = [c + (None,) for c in (
            (False, 1024, True, False), (True, 1024, True, False), (False, 256, True, False),
            (True, 256, True, False), (False, 1024, False, True), (True, 1024, False, True),
            (True, 1024, False, False))]
    for half, chunk, hip, cl, fused in configs:
        extra = {"channels_last": cl} if kind in ("osnet", "mobilenetv2") else {}
        if kind == "mobilenetv2":
            extra["fused"] = bool(fused)
        if kind == "lmbn":
            extra = {"channels_last": cl}
            if hip:
                extra["fused_neck"] = bool(fused)
        net = cls(args.variant, None, device="cuda:0", half=half, chunk=chunk, hip=hip, **extra)
        reid = ReIDDetectMultiBackend(None, device=0, fp16=half, model=net)
        crops = reid.preprocess(boxes, img)
        if half:
            crops = crops.half()
        for _ in range(3):
            net(crops)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.steps):
            net(crops)
        e1.record()
        torch.cuda.synchronize()
        net_ms = e0.elapsed_time(e1) / args.steps
        reid.get_features(boxes, img)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            reid.get_features(boxes, img)
        e2e_ms = 1000 * (time.perf_counter() - t0) / args.steps
        print(json.dumps({"metric": label + " ReID crops/s",
                          "variant": args.variant, "fused": fused,
                          "dtype": "f16" if half else "f32", "crops": n, "chunk": chunk,
                          "layout": "nhwc" if cl else "nchw", "hip_blocks": hip,
                          "network_ms": net_ms, "network_crops_per_s": n / (net_ms * 1e-3),
                          "get_features_ms": e2e_ms,
                          "get_features_crops_per_s": n / (e2e_ms * 1e-3),
                          "note": "get_features: host image -> device, crops, network, global "
                                  "norm, features back to the host (synchronous)"}))


if __name__ == "__main__":
    main()
