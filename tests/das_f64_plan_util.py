"""Shared by the CPU and the GPU check of the launch decision of das in double (csrc/das_f64_plan.hpp das_f64_decide, csrc/geometry.hpp
das_f64_slots): both through tests/host_emul (integers only), and the decision formatted in Python into the kernel names that
bf_trace_begin / bf_trace_end report."""
import ctypes as C

import numpy as np

PATHS = ("chain", "frame_pair", "ring", "transpose", "mic_pair")   # DasF64Path's order
FRAME_PAIR_PATHS = ("frame_pair", "ring", "transpose")
PLAN = ("n_levels",) + tuple(f"cnt{i}" for i in range(8)) + tuple(f"size{i}" for i in range(8)) + ("n_chunks", "grid")   # DasSchedPlan
DAS_F64_SWITCHES = dict(das_il_ring=1, sched=b"")   # switches.hpp defaults (b"" = BF_DAS_F64_SCHED unset)


def das_plan_levels(lib, n_frames, n_streams, n_cus, sched=b""):
    """das_f64_plan's own value."""
    out = (C.c_long * len(PLAN))()
    lib.emul_das_plan_levels.restype = None
    lib.emul_das_plan_levels.argtypes = [C.c_long, C.c_int, C.c_int, C.c_char_p, C.c_void_p]
    lib.emul_das_plan_levels(n_frames, n_streams, n_cus, sched, out)
    return dict(zip(PLAN, out))


def das_f64_decide(lib, layout, n_mics, n_streams=1, n_frames=96, n_cus=256, mic0_unit=True, n_tr=None, tables=True, das_il_ring=1, sched=b""):
    """The decision as a dict: path (a name of PATHS), run_frames, runs_per_stream, scratch_bytes, writes_hist, plan (as das_plan_levels).
    n_tr defaults to every microphone past 0."""
    n_tr = n_mics - 1 if n_tr is None else n_tr
    vin = (C.c_long * 9)(layout, n_mics, n_streams, n_frames, n_cus, int(mic0_unit), n_tr, int(tables), das_il_ring)
    out = (C.c_long * (5 + len(PLAN)))()
    lib.emul_das_f64_decide.restype = None
    lib.emul_das_f64_decide.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p]
    lib.emul_das_f64_decide(vin, sched, out)
    return dict(path=PATHS[out[0]], run_frames=out[1], runs_per_stream=out[2], scratch_bytes=out[3], writes_hist=bool(out[4]),
                plan=dict(zip(PLAN, out[5:])))


def das_f64_slots(lib, mics, theta, zero_row0=False, sample_rate=48000.0):
    """das_f64_slots of the das steering table a cold handle builds for the microphones [(x, y), ...] at N = 1024."""
    mx = np.array([m[0] for m in mics], dtype=np.float64)
    my = np.array([m[1] for m in mics], dtype=np.float64)
    out = (C.c_long * 11)()
    lib.emul_das_f64_slots.restype = None
    lib.emul_das_f64_slots.argtypes = [C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_double, C.c_int, C.c_void_p]
    lib.emul_das_f64_slots(len(mics), sample_rate, mx.ctypes.data_as(C.c_void_p), my.ctypes.data_as(C.c_void_p), theta, int(zero_row0), out)
    return dict(mic0_unit=bool(out[0]), n_tr=out[1], extra_mic=out[2], slot_mic=list(out[3:11]))


def params_decide(lib, p, n_frames, n_cus, layout=0, streams=1, **sw):
    """The decision for one batch of a beamform_amd.params dict on a cold handle, as BinPipelineImpl takes it: the tables exist on the
    tuned shape only (period 512, up to 8 microphones), and only there is the steering summary computed."""
    tuned = p["hop"] == 512 and p["n_mics"] <= 8
    sl = das_f64_slots(lib, p["mics"], p["theta"], sample_rate=p["sample_rate"]) if tuned else dict(mic0_unit=False, n_tr=0)
    return das_f64_decide(lib, layout, p["n_mics"], streams, n_frames, n_cus, sl["mic0_unit"], sl["n_tr"], tuned, **{**DAS_F64_SWITCHES, **sw})


def das_f64_kernels(d):
    """The decision's kernels in launch order, named as the launch trace (and docs/DISPATCH.md) prints them; not for the chain."""
    return {"frame_pair": ["das_f64_sched_kernel", "das_f64_pair_kernel"],
            "ring": ["das_f64_sched_kernel", "das_f64_ring_kernel"],
            "transpose": ["interleaved_to_planar_kernel", "interleaved_to_planar_kernel", "das_f64_sched_kernel", "das_f64_pair_kernel"],
            "mic_pair": ["das_f64_w64_kernel<1>"]}[d["path"]]
