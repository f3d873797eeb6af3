#!/usr/bin/env python3
"""Timings of steering tracks (bf_track_*) for EXPERIMENTS.md.  Needs a GPU; nothing here is asserted.

  python tools/track_bench.py batch [--parent-lib PATH] [--frames 65536] [--repeats 3]
      das in double, 8 microphones: a tracked batch with (a) a constant track and (b) a new angle every 16 frames (a random walk over
      37 angles) against the UNTRACKED batch through the same fused front (BF_FUSED_BINS=2: the one-launch kernel declines, the chain
      stays fused).  With --parent-lib the untracked batch runs on that build of the library (the parent commit's), otherwise on this
      one.  Every run is a child process (the switch is read once per process); the children alternate, each prints the milliseconds
      per call of several timed blocks (device events around the enqueues, then a synchronise) and its launch trace.
  python tools/track_bench.py loop [--frames 65536] [--block 16]
      controllers.follow_doa (one host round trip per block) against controllers.follow_doa_device (three enqueues): wall time with
      a synchronise.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _child(mode, frames, blocks, iters):
    import numpy as np
    import torch
    from beamform_amd import capi
    from beamform_amd.params import make_params
    M, H = 8, 512
    p = make_params("das", n_mics=M, theta=20.0)
    bf = capi.Beamformer(p, das_impl=capi.BF_DAS_F64)
    g = torch.Generator(device="cuda").manual_seed(1)
    x = (torch.rand((M, frames * H), generator=g, device="cuda", dtype=torch.float32) - 0.5) * 0.5
    y = torch.empty((frames * H,), dtype=torch.float32, device="cuda")
    angles = np.linspace(-90.0, 90.0, 37)
    if mode == "const":
        trk = np.full(frames, 18, np.int32)
    elif mode == "walk":
        rng = np.random.default_rng(2)
        steps = rng.choice([-1, 1], size=(frames + 15) // 16)
        pos, walk = 18, []
        for s in steps:  # reflect at the ends: a new angle at every step
            pos = pos + s if 0 <= pos + s < 37 else pos - s
            walk.append(pos)
        trk = np.repeat(np.array(walk, np.int32), 16)[:frames]
    else:
        trk = None
    if trk is not None:
        bf.set_track_angles(angles)
        td = torch.from_numpy(trk).cuda()

    def run():
        if trk is None:
            bf.process_device(x.data_ptr(), frames, y.data_ptr())
        else:
            bf.process_device_tracked(x.data_ptr(), frames, y.data_ptr(), td.data_ptr())

    with capi.launch_trace() as tr:
        run()
    for _ in range(3):
        run()
    torch.cuda.synchronize()
    ms = []
    for _ in range(blocks):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            run()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / iters)
    bf.close()
    print(json.dumps({"mode": mode, "lib": capi.LIB_PATH, "frames": frames, "ms": [round(v, 4) for v in ms], "kernels": tr.kernels}))


def _batch(a):
    runs = [("untracked", a.parent_lib), ("const", None), ("walk", None)]
    for r in range(a.repeats):
        for mode, lib in runs:
            env = dict(os.environ, BF_FUSED_BINS="2")
            if lib:
                env["BFCORE_LIB"] = os.path.abspath(lib)
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "child", "--mode", mode, "--frames", str(a.frames),
                                  "--blocks", str(a.blocks), "--iters", str(a.iters)], env=env, capture_output=True, text=True, timeout=600)
            line = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
            print(f"repeat {r} {mode:9s} " + (line[-1] if line else f"FAILED rc={out.returncode} {out.stderr[-400:]}"), flush=True)
            if out.returncode != 0:
                return 1
    return 0


def _loop(a):
    import numpy as np
    import torch
    from beamform_amd import capi
    from beamform_amd.controllers import DoaTheta, follow_doa, follow_doa_device
    from beamform_amd.params import make_params
    M, H, W, F = 8, 512, a.block, a.frames
    p = make_params("das", n_mics=M, theta=0.0)
    grid = np.arange(-180.0, 180.0)
    x = (np.random.default_rng(3).random((M, F * H), dtype=np.float32) - 0.5) * 0.5
    for name in ("follow_doa_device", "follow_doa", "follow_doa_device", "follow_doa"):
        node, doa = capi.Beamformer(p, das_impl=capi.BF_DAS_F64), capi.Doa(p, grid, 100.0, 16000.0, W)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if name == "follow_doa":
            _, pub = follow_doa(node, doa, x, W, DoaTheta(grid))
        else:
            _, pub = follow_doa_device(node, doa, x, W)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        node.close()
        doa.close()
        print(json.dumps({"loop": name, "frames": F, "block": W, "seconds": round(dt, 4), "published": len(pub)}), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", choices=["batch", "loop", "child"])
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--frames", type=int, default=65536)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--blocks", type=int, default=5, help="timed blocks per child")
    ap.add_argument("--iters", type=int, default=10, help="calls per timed block")
    ap.add_argument("--block", type=int, default=16, help="loop: frames per DOA block")
    ap.add_argument("--mode", default="untracked", choices=["untracked", "const", "walk"])
    a = ap.parse_args()
    if a.what == "child":
        return _child(a.mode, a.frames, a.blocks, a.iters)
    return _batch(a) if a.what == "batch" else _loop(a)


if __name__ == "__main__":
    sys.exit(main() or 0)
