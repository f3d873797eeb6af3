"""Shared by the CPU and the GPU check of the chain's launch plan (csrc/chain_plan.hpp): the plan through tests/host_emul's
emul_chain_plan (integers only), formatted in Python into the kernel names that bf_trace_begin / bf_trace_end report."""
import ctypes as C
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODES = ("das", "mvdr", "lcmv", "gss", "phase", "phasempf", "mcra", "gsc")
ALGO = {n: i for i, n in enumerate(NODES)}                     # bf_algo
CHAIN_SWITCHES = dict(fused_bins=1, stft_small=1, stft_split=1, mvdr_group=0, gss_group=-1, gsc_serial=0)   # switches.hpp defaults
SHAPE = ("algo", "n_fft", "layout", "n_mics", "n_streams", "n_dirs", "kp1", "past_windows", "precision", "dump", "n_frames", "n_cus",
         "gsc_filter_size", "smooth_size", "band_yh_lo", "band_yh_hi", "aligned16") + tuple(CHAIN_SWITCHES)                # ChainShape's order
PLAN = ("algo", "layout", "front", "z48", "bins", "mp", "km", "wps", "rec", "expand", "istft", "tail", "t0", "t1", "t2", "yh32", "mpf32",
        "band_rows", "yh_lo", "yh_hi", "z_bytes", "yh_bytes", "yraw_elems", "frames_elems", "fused")
SHAPE_DEFAULTS = dict(layout=0, n_streams=1, n_dirs=1, kp1=1, past_windows=10, precision=0, dump=False, gsc_filter_size=128, smooth_size=3,
                      band_yh_lo=0, band_yh_hi=0, aligned16=True, **CHAIN_SWITCHES)   # make_params' values


def chain_plan(lib, **shape):
    s = {**SHAPE_DEFAULTS, **shape}
    assert set(s) == set(SHAPE), set(s) ^ set(SHAPE)
    vin = (C.c_long * len(SHAPE))(*[int(s[k]) for k in SHAPE])
    out = (C.c_long * len(PLAN))()
    lib.emul_chain_plan.restype = None
    lib.emul_chain_plan.argtypes = [C.c_void_p, C.c_void_p]
    lib.emul_chain_plan(vin, out)
    return dict(zip(PLAN, out))


def chain_kernels(d, nfft):
    """The plan's kernels in launch order, named as the launch trace (and docs/DISPATCH.md) prints them."""
    L, mp, km, algo = d["layout"], d["mp"], d["km"], d["algo"]
    z48, z128 = ("true", "false") if d["z48"] else ("false", "true")
    k = []
    if d["front"] <= 2:
        k.append(f"{('stft_kernel', 'stft_small_kernel', 'stft_wave2048_kernel')[d['front']]}<{L}, {z48}>")
    elif d["front"] == 3:
        k.append(f"stft_generic_kernel<{L}>")
    else:
        k.append(f"{('stft_bins_w64_kernel', 'stft_bins_small_kernel', 'stft_bins_split_kernel')[d['front'] - 4]}<{L}, {mp}, {algo}>")
    k.append({0: f"fused_tail_kernel<{mp}, {algo}>", 1: f"pointwise_bins_kernel<{mp}, {algo}>", 2: f"mpf_mask_kernel<{mp}>", 3: "mcra_node_kernel",
              4: "gsc_align_kernel", 5: f"mvdr_fast_kernel<{mp}, {km}, {z128}>", 6: f"cov2d_kernel<{km}, {d['wps']}, {z128}>",
              7: f"mvdr_lcmv_kernel<{mp}, {km}>", 8: f"gss_kernel<{mp}, {km}>", 9: f"gss_lane_kernel<{mp}, {km}>"}[d["bins"]])
    k += {0: [], 1: ["mpf_recursion_kernel"], 2: ["mpf_rec_istft_kernel"]}[d["rec"]]
    k += ["expand_spectrum_kernel"] if d["expand"] else []
    k += {0: [], 1: [f"istft_w64_kernel<{'true' if d['band_rows'] else 'false'}>"], 2: ["istft32_kernel"], 3: ["istft_small_kernel"],
          4: ["istft_split_kernel"], 5: ["istft_generic_kernel", "ola_generic_kernel"]}[d["istft"]]
    t0, t1, t2 = d["t0"], d["t1"], d["t2"]
    k += {0: [], 1: [f"smooth4_kernel<{t0}>", "smooth_state_kernel"], 2: ["smooth_kernel", "smooth_state_kernel"], 3: [f"gsc_nlms_kernel<{t0}, {t1}>"],
          4: [f"gsc_nlms_par_kernel<{t0}, {t1}>"], 5: [f"gsc_nlms_mw_kernel<{t0}, {t1}, {t2}>"]}[d["tail"]]
    return [f"n{nfft}::{n}" for n in k]


def band_limits(lib, algo, nfft, freq_min, freq_max, sample_rate=48000.0):
    """The handle's band_yh_lo / band_yh_hi (csrc/chain_geom.hpp band_plan, through emul_band_plan): the in-band problems of mvdr / lcmv
    past problem 0, when the band ends below the Nyquist problems; (1, 0) for an empty band; every problem otherwise.
    (tests/chain_geom_ref.py restates the scan on its own; tests/test_chain_geom_cpu.py compares the two.)"""
    out = (C.c_long * 12)()
    lib.emul_band_plan.restype = None
    lib.emul_band_plan.argtypes = [C.c_int, C.c_double, C.c_double, C.c_double, C.c_int, C.c_void_p]
    lib.emul_band_plan(nfft, sample_rate, freq_min, freq_max, ALGO[algo], out)
    return out[2], out[3]


def params_plan(lib, p, n_frames, n_cus, layout=0, streams=1, dirs=1, dump=False, mixed=False, **sw):
    """The plan of one batch of a beamform_amd.params dict."""
    algo, nfft = p["algo"], 2 * p["hop"]
    lo, hi = band_limits(lib, algo, nfft, p["freq_min"], p["freq_max"], p["sample_rate"])
    kp1 = len(p["interf"]) + 1 if algo in ("lcmv", "gss") else 1
    return chain_plan(lib, algo=ALGO[algo], n_fft=nfft, layout=layout, n_mics=p["n_mics"], n_streams=streams, n_dirs=dirs, kp1=kp1,
                      past_windows=p["past_windows"], precision=int(mixed), dump=dump, n_frames=n_frames, n_cus=n_cus,
                      gsc_filter_size=p["gsc_filter_size"], smooth_size=p["smooth_size"], band_yh_lo=lo, band_yh_hi=hi, **sw)


def dispatch_rows():
    rows = []
    for line in open(os.path.join(ROOT, "docs", "DISPATCH.md")):
        c = [f.strip() for f in line.strip().strip("|").split("|")]
        if len(c) == 7 and c[1].isdigit():
            rows.append(c[:6] + [c[6].strip("`")])
    return rows


def row_plan(lib, row, n_frames, n_cus):
    """The plan of a docs/DISPATCH.md row (tools/dispatch_table.py: make_params' defaults; 2 interferers = -60 and 90 degrees ...)."""
    from beamform_amd.params import make_params
    node, period, layout, mics, dirs, dump, _ = row
    parts = [s.strip() for s in node.split(",")]
    algo = parts[0].split(" ")[0]
    n_interf = next((int(s.split()[0]) for s in parts if "interferer" in s), 0)
    streams = next((int(s.split()[0]) for s in parts if "streams" in s), 1)
    M = int(mics)
    over = {"mics": [(0.2, 0.0)] * M} if M > 16 else {}
    p = make_params(algo, n_mics=M, hop=int(period), interf=[10.0 * i for i in range(n_interf)], **over)
    d = params_plan(lib, p, n_frames, n_cus, layout={"planar": 0, "[sample][mic]": 1}[layout], streams=streams, dirs=int(dirs), dump=dump == "yes",
                    mixed="mixed precision" in parts)
    return d, 2 * int(period)
