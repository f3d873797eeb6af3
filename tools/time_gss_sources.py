#!/usr/bin/env python3
"""gss with R separated sources per beam: ms per batch through bf_time_batch_device.

  time_gss_sources.py [--rows 1,3] [--postfilter 0] [--mics 8] [--interf 2] [--streams 256] [--frames 256] [--hop 512] [--runs 3] [--iters 10]

One line per (rows, run): the mean over `iters` calls between two events, after five warm-up batches; uniform noise opens every gate
(the worst case: the demixing update runs in every bin).  R = 1 is the node as it always was -- BFCORE_LIB=<another build> times the
same shape on that build for an A/B in one session (a build without the field runs R = 1 only).  --postfilter 0,1 times every row
count without and with the multi-source post-filter (bf_config.gss_postfilter), alternating inside a run."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from beamform_amd import capi  # noqa: E402
from beamform_amd.params import make_params  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rows", default="1,3")
ap.add_argument("--postfilter", default="0")
ap.add_argument("--mics", type=int, default=8)
ap.add_argument("--interf", type=int, default=2)
ap.add_argument("--streams", type=int, default=256)
ap.add_argument("--frames", type=int, default=256)
ap.add_argument("--hop", type=int, default=512)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--iters", type=int, default=10)
a = ap.parse_args()

angles = (-60.0, 90.0, 150.0, 120.0, -120.0, 45.0, -45.0)[:a.interf]
p = make_params("gss", n_mics=a.mics, hop=a.hop, interf=angles)
S, F, H = a.streams, a.frames, a.hop
x = torch.rand((S, a.mics, F * H), device="cuda") - 0.5
st = torch.cuda.current_stream().cuda_stream
has_field = any(n == "gss_out_sources" for n, _ in capi.BfConfig._fields_)
print(f"library {capi.LIB_PATH}")
for R in [int(v) for v in a.rows.split(",")]:
    if R > 1 and not has_field:
        print(f"rows={R}: this binding has no gss_out_sources")
        continue
    pfs = [int(v) for v in a.postfilter.split(",")]
    bfs = {pf: capi.Beamformer(p, n_streams=S, **({"gss_out_sources": R} if R > 1 else {}), **({"gss_postfilter": 1} if pf else {})) for pf in pfs}
    y = torch.empty((bfs[pfs[0]].n_out, F * H), device="cuda")
    for run in range(a.runs):
        for pf in pfs:
            bf = bfs[pf]
            for _ in range(5):
                bf.process_device(x.data_ptr(), F, y.data_ptr(), 0, st)
            torch.cuda.synchronize()
            with capi.launch_trace() as tr:
                bf.process_device(x.data_ptr(), F, y.data_ptr(), 0, st)
            torch.cuda.synchronize()
            ms, _ = bf.time_device(x.data_ptr(), F, y.data_ptr(), a.iters, st)
            print(f"gss M={a.mics} K={a.interf} {S} streams x {F} frames hop {H} rows={R} postfilter={pf} run {run}: {ms:.3f} ms  "
                  f"[{' + '.join(k.split('::')[-1] for k in tr.kernels)}]", flush=True)
    for bf in bfs.values():
        bf.close()
