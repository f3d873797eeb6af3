#!/usr/bin/env python3
"""The multi-source loop with and without the host round trip: median wall ms per recording of controllers.follow_sources_tracked (maps
to the host, numpy picker, track back up) and controllers.follow_sources_device (four enqueues, nothing in between), in one session on
tools/time_doa.py's shape: 65 536 frames, 8 microphones, hop 512, 72 angles, W = 16, Capon, lcmv with one interferer.  Both take x on
the host and return y on the host, so both figures include the same upload and download.  Then the loop's own enqueues on resident
buffers, each between a pair of HIP events on the stream.  Prints one JSON line per figure.
  time_follow_sources.py [runs] [--frames F]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from beamform_amd import capi  # noqa: E402
from beamform_amd.controllers import DoaSources, follow_sources_device, follow_sources_tracked  # noqa: E402
from beamform_amd.params import AIRA16_XY, make_params  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("runs", nargs="?", type=int, default=20)
ap.add_argument("--frames", type=int, default=65536)
args = ap.parse_args()
F, M, HOP, W, D, K, MIN_SEP = args.frames, 8, 512, 16, 72, 2, 30.0
runs, nb = args.runs, args.frames // W
shape = {"frames": F, "mics": M, "hop": HOP, "W": W, "angles": D, "k": K, "runs": runs}
angles = np.linspace(-180.0, 180.0, D, endpoint=False)
x = (torch.rand((M, F * HOP)) - 0.5).numpy()
doa = capi.Doa(make_params("das", n_mics=M, hop=HOP, mics=AIRA16_XY[:M]), angles, 100.0, 16000.0, W)
doa.set_method("capon")
node = capi.Beamformer(make_params("lcmv", n_mics=M, hop=HOP, mics=AIRA16_XY[:M], theta=0.0, interf=[120.0]))


def host_loop():
    return follow_sources_tracked(node, doa, x, W, DoaSources(angles, K, MIN_SEP))


def device_loop():
    return follow_sources_device(node, doa, x, W, K, MIN_SEP)


wall = {"follow_sources_tracked": [], "follow_sources_device": []}
for fn in (host_loop, device_loop):  # warm-up: scratch, tables, the allocator's pools
    fn()
for _ in range(runs):  # alternating, so that a drift of the machine lands on both
    for name, fn in (("follow_sources_tracked", host_loop), ("follow_sources_device", device_loop)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        wall[name].append(1e3 * (time.perf_counter() - t0))
for name, ts in wall.items():
    print(json.dumps(dict(shape, op=name, median_ms=round(float(np.median(ts)), 3), min_ms=round(float(np.min(ts)), 3),
                          max_ms=round(float(np.max(ts)), 3))), flush=True)

# the enqueues on resident buffers
s = torch.cuda.current_stream()
st = s.cuda_stream
xd, ad = torch.from_numpy(x).cuda(), torch.from_numpy(angles).cuda()
maps = torch.empty((nb, D), dtype=torch.float64, device="cuda")
picks = torch.empty((nb, K), dtype=torch.int32, device="cuda")
carry = torch.full((2,), -1, dtype=torch.int32, device="cuda")
track = torch.empty((nb * W, 2), dtype=torch.int32, device="cuda")
yd = torch.empty((F * HOP,), dtype=torch.float32, device="cuda")
steps = [
    ("bf_doa_process_device", lambda: doa.process_device(xd.data_ptr(), F, maps.data_ptr(), 0, st)),
    ("bf_doa_pick_device", lambda: capi.doa_pick_device(maps.data_ptr(), ad.data_ptr(), D, 1, nb, K, MIN_SEP, 0.0, picks.data_ptr(), st)),
    ("bf_ctrack_from_picks_device", lambda: capi.ctrack_from_picks_device(picks.data_ptr(), maps.data_ptr(), D, K, 1, nb, W, 1, 0.0, 2,
                                                                          carry.data_ptr(), track.data_ptr(), st)),
    ("bf_process_batch_device_ctracked", lambda: node.process_device_ctracked(xd.data_ptr(), F, yd.data_ptr(), track.data_ptr(), 2, 0, st)),
]
ms = {name: [] for name, _ in steps}
for it in range(runs + 2):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(steps) + 1)]
    ev[0].record(s)
    for i, (_, fn) in enumerate(steps):
        fn()
        ev[i + 1].record(s)
    ev[-1].synchronize()
    if it >= 2:
        for i, (name, _) in enumerate(steps):
            ms[name].append(ev[i].elapsed_time(ev[i + 1]))
for name, ts in ms.items():
    print(json.dumps(dict(shape, op=name, median_ms=round(float(np.median(ts)), 4), min_ms=round(float(np.min(ts)), 4))), flush=True)
# the two track builders side by side, each launch alone between a pair of HIP events, in alternation: the tool's own shape (one stream,
# the recording's blocks) and 256 streams x 256 blocks.  bf_ctrack_assign_device walks a stream's blocks in order with one wavefront;
# bf_ctrack_from_picks_device takes 64 blocks per step.
for S_b, nb_b, m_b in ((1, nb, maps), (256, 256, None)):
    if m_b is None:
        m_b = torch.rand((S_b, nb_b, D), dtype=torch.float64, device="cuda")
    pk = torch.empty((S_b, nb_b, K), dtype=torch.int32, device="cuda")
    capi.doa_pick_device(m_b.data_ptr(), ad.data_ptr(), D, S_b, nb_b, K, MIN_SEP, 0.0, pk.data_ptr(), st)
    cr = torch.full((S_b, 2), -1, dtype=torch.int32, device="cuda")
    state = torch.full((S_b, 2, capi.BF_ASSIGN_STATE_INTS), -1, dtype=torch.int32, device="cuda")
    tk = torch.empty((S_b, nb_b * W, 2), dtype=torch.int32, device="cuda")
    act = torch.empty((S_b, nb_b, 2), dtype=torch.int32, device="cuda")
    builders = [
        ("bf_ctrack_from_picks_device", lambda: capi.ctrack_from_picks_device(pk.data_ptr(), m_b.data_ptr(), D, K, S_b, nb_b, W, 1, 0.0, 2,
                                                                              cr.data_ptr(), tk.data_ptr(), st)),
        ("bf_ctrack_assign_device", lambda: capi.ctrack_assign_device(pk.data_ptr(), m_b.data_ptr(), ad.data_ptr(), D, K, S_b, nb_b, W, 1, 0.0,
                                                                      20.0, 2, 8, 2, state.data_ptr(), tk.data_ptr(), act.data_ptr(), st)),
    ]
    bms = {name: [] for name, _ in builders}
    for it in range(runs + 2):
        for name, fn in builders:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            fn()
            e1.record(s)
            e1.synchronize()
            if it >= 2:
                bms[name].append(e0.elapsed_time(e1))
    for name, ts in bms.items():
        print(json.dumps(dict(shape, op=name + " alone", streams=S_b, blocks=nb_b, median_ms=round(float(np.median(ts)), 4),
                              min_ms=round(float(np.min(ts)), 4))), flush=True)
# the host's share of the round trip, on its own: the numpy picker and schedule over the same maps
from beamform_amd.controllers import sources_track  # noqa: E402
mh = maps.cpu().numpy()
t0 = time.perf_counter()
sources_track(mh, DoaSources(angles, K, MIN_SEP), W, 2, 1)
print(json.dumps(dict(shape, op="sources_track (numpy)", ms=round(1e3 * (time.perf_counter() - t0), 3))), flush=True)
node.close()
doa.close()
