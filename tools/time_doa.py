#!/usr/bin/env python3
"""bf_doa: median ms per 65 536-frame batch (8 microphones, hop 512, band 100-16 000 Hz, W = 16) at 72 and 360 angles, HIP events
around each bf_doa_process_device call on one stream, >= 20 timed runs after warm-up.  Prints one JSON line per shape.
  time_doa.py [runs] [--method srp_phat|capon|music|both|all] [--mics M] [--frames F] [--angles D ...] [--sources N]
both: srp_phat and capon; all: the three methods.  --sources: MUSIC's signal subspace (default 2)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from beamform_amd.capi import Doa  # noqa: E402
from beamform_amd.params import AIRA16_XY, make_params  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("runs", nargs="?", type=int, default=20)
ap.add_argument("--method", choices=("srp_phat", "capon", "music", "both", "all"), default="srp_phat")
ap.add_argument("--mics", type=int, default=8)
ap.add_argument("--frames", type=int, default=65536)
ap.add_argument("--angles", type=int, nargs="+", default=[72, 360])
ap.add_argument("--sources", type=int, default=2)
args = ap.parse_args()
F, M, HOP, W = args.frames, args.mics, 512, 16
METHODS = {"both": ("srp_phat", "capon"), "all": ("srp_phat", "capon", "music")}.get(args.method, (args.method,))
runs = args.runs
x = torch.rand((M, F * HOP), device="cuda") - 0.5
s = torch.cuda.current_stream()
for D, method in ((D, m) for D in args.angles for m in METHODS):
    angles = np.linspace(-180.0, 180.0, D, endpoint=False)
    doa = Doa(make_params("das", n_mics=M, hop=HOP, mics=AIRA16_XY[:M]), angles, 100.0, 16000.0, W)
    doa.set_method(method)
    doa.set_sources(args.sources)
    m = torch.empty((F // W, D), dtype=torch.float64, device="cuda")
    k = torch.empty((F // W,), dtype=torch.int32, device="cuda")
    for _ in range(3):
        doa.process_device(x.data_ptr(), F, m.data_ptr(), k.data_ptr(), s.cuda_stream)
    torch.cuda.synchronize()
    ts = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        doa.process_device(x.data_ptr(), F, m.data_ptr(), k.data_ptr(), s.cuda_stream)
        e1.record(s)
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    doa.close()
    print(json.dumps({"op": "bf_doa", "method": method, "frames": F, "mics": M, "hop": HOP, "W": W, "angles": D, "runs": runs,
                      "median_ms": round(float(np.median(ts)), 4), "min_ms": round(float(np.min(ts)), 4)}), flush=True)
