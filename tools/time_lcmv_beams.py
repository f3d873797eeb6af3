#!/usr/bin/env python3
"""lcmv with a beam per constraint column (bf_config.lcmv_out_beams): ms per batch through bf_time_batch_device.

  time_lcmv_beams.py [--mics 16] [--interf 3] [--frames 32768] [--hop 512] [--variants one,rows,handles] [--rounds 5] [--iters 5]
                     [--out record.json]

The variants of one shape, interleaved round by round in one process on one device (uniform noise opens every gate):
  one      a handle with one output row: the node as it always was
  rows     a handle with lcmv_out_beams = K + 1: every beam out of one pass
  handles  K + 1 one-row handles, handle r with `angle` and interferer r exchanged: the same K + 1 signals out of K + 1 passes
           (the sum of their times is reported)
Per variant: every round's mean over `iters` calls, the median and the minimum over the rounds, the spread (max - min) / median,
and the kernels of one batch.  BFCORE_LIB=<another build> times `one` on that build for an A/B against another commit in the same
session (a build without the field runs `one` only)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from beamform_amd import capi  # noqa: E402
from beamform_amd.params import make_params  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--mics", type=int, default=16)
ap.add_argument("--interf", type=int, default=3)
ap.add_argument("--frames", type=int, default=32768)
ap.add_argument("--hop", type=int, default=512)
ap.add_argument("--variants", default="one,rows,handles")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--iters", type=int, default=5)
ap.add_argument("--out", default="")
a = ap.parse_args()

theta = 20.0
interf = list((-60.0, 90.0, 150.0, -120.0, 60.0, -150.0, 120.0)[:a.interf])
M, K, F, H = a.mics, a.interf, a.frames, a.hop
x = torch.rand((M, F * H), device="cuda") - 0.5
y = torch.empty((K + 1, F * H), device="cuda")
st = torch.cuda.current_stream().cuda_stream


def node(th, it, rows=1):
    p = make_params("lcmv", n_mics=M, hop=H, theta=th, interf=it)
    return capi.Beamformer(p, **({"lcmv_out_beams": rows} if rows > 1 else {}))


handles = {}
for v in a.variants.split(","):
    if v == "one":
        handles[v] = [node(theta, interf)]
    elif v == "rows":
        handles[v] = [node(theta, interf, K + 1)]
    elif v == "handles":
        handles[v] = [node(theta, interf)]
        for r in range(1, K + 1):
            it = list(interf)
            it[r - 1] = theta
            handles[v].append(node(interf[r - 1], it))
    else:
        raise SystemExit(f"unknown variant {v}")

rec = dict(library=capi.LIB_PATH, mics=M, interferers=K, frames=F, hop=H, iters=a.iters, device=torch.cuda.get_device_name(0), variants={})
for v, hs in handles.items():
    for bf in hs:
        for _ in range(2):
            bf.process_device(x.data_ptr(), F, y.data_ptr(), 0, st)
    with capi.launch_trace() as tr:
        hs[0].process_device(x.data_ptr(), F, y.data_ptr(), 0, st)
    torch.cuda.synchronize()
    rec["variants"][v] = dict(kernels=[k.split("::")[-1] for k in tr.kernels], ms=[], kernel_ms=[])
for rnd in range(a.rounds):
    for v, hs in handles.items():
        ms = msk = 0.0
        for bf in hs:
            m, k = bf.time_device(x.data_ptr(), F, y.data_ptr(), a.iters, st)
            ms, msk = ms + m, msk + k
        rec["variants"][v]["ms"].append(ms)
        rec["variants"][v]["kernel_ms"].append(msk)
for v, d in rec["variants"].items():
    d["median_ms"], d["min_ms"] = statistics.median(d["ms"]), min(d["ms"])
    d["spread"] = (max(d["ms"]) - min(d["ms"])) / d["median_ms"]
    d["median_kernel_ms"] = statistics.median(d["kernel_ms"])
    print(f"lcmv M={M} K={K} {F} frames hop {H} {v}: median {d['median_ms']:.3f} ms, min {d['min_ms']:.3f}, spread {100 * d['spread']:.1f} %, "
          f"dominant kernel {d['median_kernel_ms']:.3f} ms  rounds {[round(m, 3) for m in d['ms']]}  [{' + '.join(d['kernels'])}]", flush=True)
for hs in handles.values():
    for bf in hs:
        bf.close()
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
