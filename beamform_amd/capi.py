"""ctypes binding of libbfcore.so (include/bfcore.h).

Thin plumbing only: device memory comes from the caller (torch tensors / raw
pointers); all compute happens in the HIP kernels behind the C ABI.  Loading
fails loudly when the library is missing -- there is no Python or CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from .params import ALGO_ID

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("BFCORE_LIB") or os.path.join(_HERE, "lib", "libbfcore.so")  # BFCORE_LIB: A/B builds of the same ABI

BF_MAX_MICS = 32
BF_MAX_INTERF = 15
BF_PLANAR, BF_INTERLEAVED = 0, 1
BF_PRECISION_REFERENCE, BF_PRECISION_MIXED = 0, 1   # bf_precision: doubles between the transforms (default) / z48 spectra + fp32 backward transform
BF_DAS_FUSED_F32, BF_DAS_F64 = 0, 1   # bf_das_impl: fp32 opt-in / double like the reference (the default, as in bf_config_init)

#: every symbol include/bfcore.h declares
EXPORTS = (
    "bf_version", "bf_strerror", "bf_last_error", "bf_device_count", "bf_config_init", "bf_config_load_yaml",
    "bf_config_parse_yaml", "bf_create", "bf_destroy", "bf_set_theta", "bf_set_interference", "bf_process_hop",
    "bf_process_batch", "bf_process_batch_device", "bf_get_weights", "bf_state_size", "bf_get_state", "bf_set_state",
    "bf_reset", "bf_reset_async", "bf_shard_halo", "bf_shard_plan", "bf_shard_run", "bf_shard_first_feed", "bf_shard_n_feed", "bf_shard_n_drop", "bf_process_batch_device_strided", "bf_kernel_timing_begin", "bf_kernel_timing_end", "bf_trace_begin", "bf_trace_end", "bf_time_batch_device", "bf_n_interferers", "bf_set_theta_dir", "bf_set_thetas", "bf_stream_rms", "bf_host_alloc", "bf_host_free",
    "bf_wav_writer_open", "bf_wav_writer_write", "bf_wav_writer_write_pcm16", "bf_wav_writer_close", "bf_float_to_pcm16",
    "bf_float_to_pcm16_device", "bf_wav_read", "bf_planar_f32_read", "bf_wav_free",
    "bf_resampler_create", "bf_resampler_set_table", "bf_resampler_reset", "bf_resampler_out_count", "bf_resampler_latency",
    "bf_resampler_process_device", "bf_resampler_process", "bf_resampler_destroy", "bf_resampler_default_table",
    "bf_resampler_set_mode", "bf_resampler_callback", "bf_resampler_callback_device",
    "bf_doa_create", "bf_doa_set_phat_floor", "bf_doa_set_method", "bf_doa_set_loading", "bf_doa_process_device", "bf_doa_process",
    "bf_doa_set_sources", "bf_doa_set_music_floor", "bf_doa_process_device_eig", "bf_doa_process_eig",
    "bf_doa_reset", "bf_doa_destroy",
    "bf_track_set_angles", "bf_process_batch_device_tracked", "bf_track_from_peaks_device",
    "bf_ctrack_set_angles", "bf_process_batch_device_ctracked",
    "bf_doa_pick_device", "bf_ctrack_from_picks_device", "bf_ctrack_assign_device",
)
BF_DOA_MAX_ANGLES = 1024
BF_DOA_SRP_PHAT, BF_DOA_CAPON, BF_DOA_MUSIC = 0, 1, 2   # bf_doa_method
BF_TRACK_MAX_ANGLES = 1024   # = BF_DOA_MAX_ANGLES: a Doa peak index is a track index
BF_DOA_MAX_PICKS = 16        # = BF_MAX_INTERF + 1: a look direction and every interferer
BF_ASSIGN_STATE_INTS = 4     # bf_ctrack_assign_device: {idx, hits, misses, out} per slot


class BfConfig(C.Structure):
    _fields_ = [
        ("algo", C.c_int), ("n_mics", C.c_int), ("hop", C.c_int), ("sample_rate", C.c_double),
        ("mic_x", C.c_double * BF_MAX_MICS), ("mic_y", C.c_double * BF_MAX_MICS), ("theta", C.c_double),
        ("n_interf", C.c_int), ("interf_angle", C.c_double * BF_MAX_INTERF), ("verbose", C.c_int),
        ("past_windows", C.c_int), ("freq_mag_threshold", C.c_double), ("freq_max", C.c_double),
        ("freq_min", C.c_double), ("out_amp", C.c_double), ("interf_angle_threshold", C.c_double),
        ("mu", C.c_double), ("lambda_", C.c_double),
        ("min_phase", C.c_double), ("mag_mult", C.c_double), ("mag_threshold", C.c_double),
        ("min_mag", C.c_double), ("smooth_size", C.c_int),
        ("mcra_alphaS", C.c_double), ("mcra_alphaD", C.c_double), ("mcra_alphaD2", C.c_double),
        ("mcra_delta", C.c_double), ("mcra_L", C.c_int),
        ("mpf_alphaS", C.c_double), ("mpf_eta", C.c_double), ("mpf_rev_gamma", C.c_double),
        ("mpf_rev_delta", C.c_double), ("noise_floor", C.c_double),
        ("out_only_noise", C.c_int), ("out_only_mcra", C.c_int),
        ("device", C.c_int), ("n_streams", C.c_int), ("layout", C.c_int), ("das_impl", C.c_int), ("precision", C.c_int), ("n_dirs", C.c_int),
        ("gsc_use_vad", C.c_int), ("gsc_vad_threshold", C.c_double), ("gsc_mu0", C.c_double), ("gsc_mu_max", C.c_double),
        ("gsc_filter_size", C.c_int),
        ("gss_out_sources", C.c_int),
        ("gss_postfilter", C.c_int),
        ("lcmv_out_beams", C.c_int),
    ]


#: defaults of parameters added after the first golden fixtures were written (launch/gsc.launch:6-11)
_LATER_KEYS = dict(gsc_use_vad=0, gsc_vad_threshold=0.1, gsc_mu0=0.0001, gsc_mu_max=0.1, gsc_filter_size=128, gss_out_sources=0,
                   gss_postfilter=0, lcmv_out_beams=0)


class BfError(RuntimeError):
    def __init__(self, code, what, detail=""):
        super().__init__(f"{what}: [{code}] {detail}")
        self.code = code


_lib = None


#: which HIP runtime libbfcore.so ended up bound to: "torch:<path>" (the wheel's copy was loaded first), "system" or "unknown"
HIP_RUNTIME_BOUND = "unknown"


def _share_torch_hip_runtime():
    """One HIP runtime per process.  A PyTorch-ROCm wheel ships its own libamdhip64.so (same soname as /opt/rocm's); if libbfcore.so
    is loaded first it brings in /opt/rocm's copy, torch then loads its own beside it, and the second runtime to initialise reports
    "no ROCm-capable device".  When torch is installed but not imported yet, load ITS runtime first (without importing torch) so that
    libbfcore.so's DT_NEEDED resolves to the copy torch will use.  BF_NO_TORCH_HIP=1 skips this (a process that never imports torch
    keeps the /opt/rocm runtime libbfcore.so was built against).  What happened is recorded in HIP_RUNTIME_BOUND; BF_HIP_DEBUG=1 also
    prints the runtime's version (that call initialises HIP, so it is made in debug runs only: load() itself stays a plain dlopen, safe
    in front of a fork and for the host-only helpers -- wav, config, pcm16)."""
    global HIP_RUNTIME_BOUND
    import sys
    if os.environ.get("BF_NO_TORCH_HIP") == "1":
        HIP_RUNTIME_BOUND = "system"
        return
    if "torch" in sys.modules:
        HIP_RUNTIME_BOUND = "torch:already imported"
        return
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        HIP_RUNTIME_BOUND = "system"
        return
    path = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(path):
        try:
            rt = C.CDLL(path, mode=C.RTLD_GLOBAL)
            HIP_RUNTIME_BOUND = "torch:" + path
            if os.environ.get("BF_HIP_DEBUG") == "1":
                v = C.c_int(0)
                if rt.hipRuntimeGetVersion(C.byref(v)) == 0:
                    print(f"[bfcore] bound to the torch wheel's HIP runtime {path} (version {v.value})", file=sys.stderr)
        except OSError:
            HIP_RUNTIME_BOUND = "system"  # not loadable on its own: libbfcore.so falls back to its RUNPATH copy
    else:
        HIP_RUNTIME_BOUND = "system"


def load():
    """dlopen libbfcore.so; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: run `make` (or __graft_entry__.build()); "
                          "beamform_amd has no CPU fallback")
    _share_torch_hip_runtime()
    L = C.CDLL(LIB_PATH)
    L.bf_version.restype = C.c_char_p
    L.bf_strerror.restype = C.c_char_p
    L.bf_strerror.argtypes = [C.c_int]
    L.bf_last_error.restype = C.c_char_p
    L.bf_last_error.argtypes = [C.c_void_p]
    L.bf_config_init.argtypes = [C.POINTER(BfConfig), C.c_int]
    L.bf_config_load_yaml.argtypes = [C.POINTER(BfConfig), C.c_char_p]
    L.bf_config_parse_yaml.argtypes = [C.POINTER(BfConfig), C.c_char_p]
    L.bf_create.argtypes = [C.POINTER(BfConfig), C.POINTER(C.c_void_p)]
    L.bf_destroy.argtypes = [C.c_void_p]
    L.bf_destroy.restype = None
    L.bf_set_theta.argtypes = [C.c_void_p, C.c_double]
    L.bf_set_theta_dir.argtypes = [C.c_void_p, C.c_int, C.c_double]
    L.bf_set_thetas.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_int]
    L.bf_stream_rms.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_double), C.c_void_p]
    L.bf_set_interference.argtypes = [C.c_void_p, C.c_uint, C.c_double]
    L.bf_n_interferers.argtypes = [C.c_void_p]
    L.bf_process_hop.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_void_p, C.c_uint32]
    L.bf_process_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    L.bf_host_alloc.restype = C.c_void_p
    L.bf_host_alloc.argtypes = [C.c_size_t]
    L.bf_host_free.argtypes = [C.c_void_p]
    L.bf_host_free.restype = None
    L.bf_process_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
    L.bf_get_weights.argtypes = [C.c_void_p, C.c_void_p]
    L.bf_state_size.restype = C.c_size_t
    L.bf_state_size.argtypes = [C.c_void_p]
    L.bf_get_state.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.bf_set_state.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.bf_reset.argtypes = [C.c_void_p]
    L.bf_reset_async.argtypes = [C.c_void_p, C.c_void_p]
    L.bf_process_batch_device_strided.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_long]
    L.bf_kernel_timing_begin.argtypes = [C.c_void_p]
    L.bf_kernel_timing_end.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int)]
    L.bf_trace_begin.argtypes = []
    L.bf_trace_end.argtypes = [C.c_char_p, C.c_size_t]
    L.bf_trace_end.restype = C.c_long
    L.bf_time_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int,
                                       C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.bf_wav_writer_open.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_void_p)]
    L.bf_wav_writer_write.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.bf_wav_writer_write_pcm16.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.bf_wav_writer_close.argtypes = [C.c_void_p]
    L.bf_float_to_pcm16.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.bf_float_to_pcm16.restype = None
    L.bf_float_to_pcm16_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    L.bf_wav_read.argtypes = [C.c_char_p, C.POINTER(C.POINTER(C.c_float)), C.POINTER(C.c_int), C.POINTER(C.c_size_t),
                              C.POINTER(C.c_int)]
    L.bf_planar_f32_read.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.POINTER(C.c_float)), C.POINTER(C.c_size_t)]
    L.bf_wav_free.argtypes = [C.POINTER(C.c_float)]
    L.bf_wav_free.restype = None
    L.bf_resampler_create.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    L.bf_resampler_set_table.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    L.bf_resampler_reset.argtypes = [C.c_void_p]
    L.bf_resampler_out_count.argtypes = [C.c_void_p, C.c_size_t]
    L.bf_resampler_out_count.restype = C.c_size_t
    L.bf_resampler_latency.argtypes = [C.c_void_p]
    L.bf_resampler_process_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_void_p]
    L.bf_resampler_process.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.bf_resampler_destroy.argtypes = [C.c_void_p]
    L.bf_resampler_destroy.restype = None
    L.bf_resampler_default_table.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    L.bf_resampler_set_mode.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.bf_resampler_callback.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.bf_resampler_callback_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p]
    L.bf_doa_create.argtypes = [C.POINTER(BfConfig), C.POINTER(C.c_double), C.c_int, C.c_double, C.c_double, C.c_int,
                                C.POINTER(C.c_void_p)]
    L.bf_doa_set_phat_floor.argtypes = [C.c_void_p, C.c_double]
    L.bf_doa_set_method.argtypes = [C.c_void_p, C.c_int]
    L.bf_doa_set_loading.argtypes = [C.c_void_p, C.c_double]
    L.bf_doa_process_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
    L.bf_doa_process.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    L.bf_doa_set_sources.argtypes = [C.c_void_p, C.c_int]
    L.bf_doa_set_music_floor.argtypes = [C.c_void_p, C.c_double]
    L.bf_doa_process_device_eig.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.bf_doa_process_eig.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
    L.bf_doa_reset.argtypes = [C.c_void_p]
    L.bf_doa_destroy.argtypes = [C.c_void_p]
    L.bf_doa_destroy.restype = None
    L.bf_track_set_angles.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_int]
    L.bf_process_batch_device_tracked.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.bf_ctrack_set_angles.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_int]
    L.bf_process_batch_device_ctracked.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    L.bf_track_from_peaks_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.c_int, C.c_int, C.c_double,
                                             C.c_void_p, C.c_void_p, C.c_void_p]
    L.bf_doa_pick_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.c_int, C.c_double, C.c_double, C.c_void_p,
                                     C.c_void_p]
    L.bf_ctrack_from_picks_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_int, C.c_int, C.c_double,
                                              C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.bf_ctrack_assign_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_int, C.c_int,
                                          C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p]
    _lib = L
    return L


# ---- rosjack output stage, file half (rosjack.cpp:189-210, 404-409) and the batch front-end ---------------------------------
class launch_trace:
    """with launch_trace() as t: ... ; t.kernels = the kernels this thread launched through the library inside the block, in launch
    order, named as rocprofv3 names them (bf_trace_begin / bf_trace_end)."""

    def __enter__(self):
        L = load()
        rc = L.bf_trace_begin()
        if rc != 0:
            raise BfError(rc, "bf_trace_begin", "a trace is already open on this thread")
        self.kernels = []
        return self

    def __exit__(self, *exc):
        L = load()
        buf = C.create_string_buffer(1 << 16)
        n = L.bf_trace_end(buf, len(buf))
        if n < 0:
            raise BfError(int(n), "bf_trace_end")
        self.kernels = [k for k in buf.value.decode().split("\n") if k]
        return False


class WavWriter:
    """sf_open(..., SFM_WRITE, WAV | PCM_16, mono) / sf_write_float per callback / sf_close."""

    def __init__(self, path: str, sample_rate: int = 48000):
        self._L = load()
        self._w = C.c_void_p()
        rc = self._L.bf_wav_writer_open(os.fsencode(path), int(sample_rate), C.byref(self._w))
        if rc:
            raise BfError(rc, "bf_wav_writer_open", self._L.bf_strerror(rc).decode())

    def write(self, samples: np.ndarray):
        a = np.ascontiguousarray(samples, np.float32)
        rc = self._L.bf_wav_writer_write(self._w, a.ctypes.data, a.size)
        if rc:
            raise BfError(rc, "bf_wav_writer_write", self._L.bf_strerror(rc).decode())

    def write_pcm16(self, pcm: np.ndarray):
        a = np.ascontiguousarray(pcm, np.int16)
        rc = self._L.bf_wav_writer_write_pcm16(self._w, a.ctypes.data, a.size)
        if rc:
            raise BfError(rc, "bf_wav_writer_write_pcm16", self._L.bf_strerror(rc).decode())

    def close(self):
        if self._w:
            rc = self._L.bf_wav_writer_close(self._w)
            self._w = None
            if rc:
                raise BfError(rc, "bf_wav_writer_close", self._L.bf_strerror(rc).decode())

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def float_to_pcm16(x: np.ndarray) -> np.ndarray:
    """The sample rule of sf_write_float on a PCM_16 file (host)."""
    a = np.ascontiguousarray(x, np.float32)
    out = np.empty(a.shape, np.int16)
    load().bf_float_to_pcm16(a.ctypes.data, out.ctypes.data, a.size)
    return out


def float_to_pcm16_device(src_ptr: int, dst_ptr: int, n: int, stream: int = 0):
    rc = load().bf_float_to_pcm16_device(src_ptr, dst_ptr, n, stream or None)
    if rc:
        raise BfError(rc, "bf_float_to_pcm16_device", load().bf_strerror(rc).decode())


def _take_planar(L, p, ch, n):
    arr = np.ctypeslib.as_array(p, shape=(ch * n,)).reshape(ch, n).copy() if ch * n else np.zeros((ch, 0), np.float32)
    L.bf_wav_free(p)
    return arr


def read_wav(path: str):
    """WAV file -> (planar float32 [channels, samples], sample_rate)."""
    L = load()
    p, ch, n, sr = C.POINTER(C.c_float)(), C.c_int(), C.c_size_t(), C.c_int()
    rc = L.bf_wav_read(os.fsencode(path), C.byref(p), C.byref(ch), C.byref(n), C.byref(sr))
    if rc:
        raise BfError(rc, "bf_wav_read", L.bf_strerror(rc).decode())
    return _take_planar(L, p, ch.value, n.value), sr.value


def read_planar_f32(path: str, n_channels: int) -> np.ndarray:
    L = load()
    p, n = C.POINTER(C.c_float)(), C.c_size_t()
    rc = L.bf_planar_f32_read(os.fsencode(path), n_channels, C.byref(p), C.byref(n))
    if rc:
        raise BfError(rc, "bf_planar_f32_read", L.bf_strerror(rc).decode())
    return _take_planar(L, p, n_channels, n.value)


# ---- rosjack output stage, sample-rate half (rosjack.cpp:159-184, 311-338) ----------------------------------------------------
class Resampler:
    """src_new(SRC_SINC_FASTEST, 1) with src_ratio = out_rate / in_rate; process() is src_process with end_of_input = 0."""

    def __init__(self, in_rate: int, out_rate: int):
        self._L = load()
        self._r = C.c_void_p()
        rc = self._L.bf_resampler_create(int(in_rate), int(out_rate), C.byref(self._r))
        if rc:
            raise BfError(rc, "bf_resampler_create", self._L.bf_strerror(rc).decode())

    def _check(self, rc, what):
        if rc:
            raise BfError(rc, what, self._L.bf_strerror(rc).decode())

    def set_table(self, coeffs: np.ndarray, index_inc: int):
        a = np.ascontiguousarray(coeffs, np.float32)
        self._check(self._L.bf_resampler_set_table(self._r, a.ctypes.data, a.size, int(index_inc)), "bf_resampler_set_table")

    def reset(self):
        self._check(self._L.bf_resampler_reset(self._r), "bf_resampler_reset")

    @property
    def latency(self) -> int:
        return self._L.bf_resampler_latency(self._r)

    def out_count(self, n_in: int) -> int:
        return self._L.bf_resampler_out_count(self._r, n_in)

    def process(self, x: np.ndarray) -> np.ndarray:
        a = np.ascontiguousarray(x, np.float32)
        n = C.c_size_t()
        out = np.empty(self.out_count(a.size), np.float32)
        self._check(self._L.bf_resampler_process(self._r, a.ctypes.data, a.size, out.ctypes.data, out.size, C.byref(n)),
                    "bf_resampler_process")
        return out[:n.value]

    def process_device(self, in_ptr: int, n_in: int, out_ptr: int, out_cap: int, stream: int = 0) -> int:
        n = C.c_size_t()
        self._check(self._L.bf_resampler_process_device(self._r, in_ptr, n_in, out_ptr, out_cap, C.byref(n), stream or None),
                    "bf_resampler_process_device")
        return n.value

    def set_mode_rosjack(self, period: int):
        """BF_RS_ROSJACK: the stage as rosjack drives it (period drops on upsampling, one block per callback); see bfcore.h."""
        self._period = int(period)
        self._check(self._L.bf_resampler_set_mode(self._r, 1, int(period)), "bf_resampler_set_mode")

    def set_mode_stream(self):
        self._check(self._L.bf_resampler_set_mode(self._r, 0, 0), "bf_resampler_set_mode")

    def callback(self, period: np.ndarray):
        """One output_to_rosjack: returns (published block or None, accepted flag)."""
        a = np.ascontiguousarray(period, np.float32)
        assert a.size == self._period
        out = np.empty(self._period, np.float32)
        em, acc = C.c_int(), C.c_int()
        self._check(self._L.bf_resampler_callback(self._r, a.ctypes.data, out.ctypes.data, C.byref(em), C.byref(acc)), "bf_resampler_callback")
        return (out if em.value else None), bool(acc.value)

    def callback_device(self, in_ptr: int, out_ptr: int, stream: int = 0):
        em, acc = C.c_int(), C.c_int()
        self._check(self._L.bf_resampler_callback_device(self._r, in_ptr, out_ptr, C.byref(em), C.byref(acc), stream or None),
                    "bf_resampler_callback_device")
        return bool(em.value), bool(acc.value)

    def close(self):
        if self._r:
            self._L.bf_resampler_destroy(self._r)
            self._r = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def resampler_default_table():
    """(built-in coefficient table, index_inc)."""
    L = load()
    inc = C.c_int()
    n = L.bf_resampler_default_table(None, 0, C.byref(inc))
    t = np.empty(n, np.float32)
    L.bf_resampler_default_table(t.ctypes.data, n, C.byref(inc))
    return t, inc.value


def config_from_params(p: dict, device: int = 0, n_streams: int = 1, layout: int = BF_PLANAR,
                       das_impl: int = BF_DAS_F64, n_dirs: int = 1, precision: int = BF_PRECISION_REFERENCE,
                       gss_out_sources: int = None, gss_postfilter: int = None, lcmv_out_beams: int = None) -> BfConfig:
    """bf_config from a beamform_amd.params dict (launch defaults first, then overrides).  gss_out_sources / gss_postfilter /
    lcmv_out_beams: the dict's value unless given."""
    L = load()
    c = BfConfig()
    rc = L.bf_config_init(C.byref(c), ALGO_ID[p["algo"]])
    if rc:
        raise BfError(rc, "bf_config_init", L.bf_strerror(rc).decode())
    c.n_mics = p["n_mics"]
    c.hop = p["hop"]
    c.sample_rate = p["sample_rate"]
    for i, (x, y) in enumerate(p["mics"]):
        c.mic_x[i], c.mic_y[i] = x, y
    c.theta = p["theta"]
    c.n_interf = len(p["interf"])
    for i, a in enumerate(p["interf"]):
        c.interf_angle[i] = a
    for k in ("past_windows", "freq_mag_threshold", "freq_max", "freq_min", "out_amp", "mu", "lambda_", "min_phase",
              "mag_mult", "mag_threshold", "min_mag", "smooth_size", "mcra_alphaS", "mcra_alphaD", "mcra_alphaD2",
              "mcra_delta", "mcra_L", "mpf_alphaS", "mpf_eta", "mpf_rev_gamma", "mpf_rev_delta", "noise_floor",
              "out_only_noise", "out_only_mcra", "gsc_use_vad", "gsc_vad_threshold", "gsc_mu0", "gsc_mu_max",
              "gsc_filter_size", "gss_out_sources", "gss_postfilter", "lcmv_out_beams"):
        setattr(c, k, p[k] if k in p else _LATER_KEYS[k])  # fixtures written before a key existed
    if gss_out_sources is not None:
        c.gss_out_sources = gss_out_sources
    if gss_postfilter is not None:
        c.gss_postfilter = gss_postfilter
    if lcmv_out_beams is not None:
        c.lcmv_out_beams = lcmv_out_beams
    c.device, c.n_streams, c.layout, c.das_impl, c.n_dirs = device, n_streams, layout, das_impl, n_dirs
    c.precision = precision
    return c


def host_array(shape, dtype=np.float32):
    """numpy array over page-locked memory from bf_host_alloc (freed when the array is collected)."""
    L = load()
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    ptr = L.bf_host_alloc(n)
    if not ptr:
        raise MemoryError("bf_host_alloc failed")
    buf = (C.c_char * n).from_address(ptr)
    arr = np.frombuffer(buf, dtype=dtype).reshape(shape)
    import weakref
    weakref.finalize(buf, L.bf_host_free, ptr)
    return arr


class Beamformer:
    """One beamformer node behind the C ABI (das|mvdr|lcmv|gss|phase|phasempf|mcra|gsc)."""

    def __init__(self, params: dict, device: int = 0, n_streams: int = 1, layout: int = BF_PLANAR,
                 das_impl: int = BF_DAS_F64, n_dirs: int = 1, precision: int = BF_PRECISION_REFERENCE, gss_out_sources: int = None,
                 gss_postfilter: int = None, lcmv_out_beams: int = None):
        """gss_out_sources = R > 1 (gss only): every beam yields its R separated sources, not only the first (bf_config.gss_out_sources);
        the outputs gain an axis of length R, innermost among the stream axes.  gss_postfilter = 1 (gss only): every separated source
        goes through the multi-source post-filter (bf_config.gss_postfilter: noise, leak of the other sources and reverberation come off
        its magnitude).  lcmv_out_beams = R > 1 (lcmv only): every beam yields R signals, row r looking at constraint column r (the look
        direction, then the interferers) with nulls on the other columns (bf_config.lcmv_out_beams); same extra axis as gss_out_sources."""
        self._L = load()
        self.cfg = config_from_params(params, device, n_streams, layout, das_impl, n_dirs, precision, gss_out_sources, gss_postfilter,
                                      lcmv_out_beams)
        self.n_dirs = max(1, n_dirs)
        self.n_rows = max(1, self.cfg.gss_out_sources, self.cfg.lcmv_out_beams)  # (bf_create refuses both above 1)
        self.n_out = n_streams * self.n_dirs * self.n_rows  # output streams: [stream][dir][row]
        self.M, self.H, self.N = params["n_mics"], params["hop"], 2 * params["hop"]
        self.S = len(params["interf"]) + 1 if params["algo"] in ("lcmv", "gss") else 1
        self.n_streams = n_streams
        self._h = C.c_void_p()
        rc = self._L.bf_create(C.byref(self.cfg), C.byref(self._h))
        if rc:
            raise BfError(rc, "bf_create", self._L.bf_last_error(None).decode())

    def close(self):
        if getattr(self, "_h", None):
            self._L.bf_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def _chk(self, rc, what):
        if rc:
            raise BfError(rc, what, (self._L.bf_last_error(self._h) or b"").decode() or self._L.bf_strerror(rc).decode())

    def set_theta(self, deg: float):
        self._chk(self._L.bf_set_theta(self._h, float(deg)), "bf_set_theta")

    def set_theta_dir(self, d: int, deg: float):
        self._chk(self._L.bf_set_theta_dir(self._h, int(d), float(deg)), "bf_set_theta_dir")

    def set_thetas(self, degs):
        """One /theta per look direction (n_dirs of them), one table rebuild."""
        a = (C.c_double * len(degs))(*[float(v) for v in degs])
        self._chk(self._L.bf_set_thetas(self._h, a, len(degs)), "bf_set_thetas")

    def stream_rms(self, y_ptr: int, n_frames: int, stream: int = 0) -> np.ndarray:
        """RMS of every output stream of a device-resident batch -> [n_streams, n_dirs] float64 ([n_streams, n_dirs, R] with
        gss_out_sources / lcmv_out_beams = R > 1)."""
        out = (C.c_double * self.n_out)()
        self._chk(self._L.bf_stream_rms(self._h, y_ptr, n_frames, out, stream or None), "bf_stream_rms")
        shape = (self.n_streams, self.n_dirs) + ((self.n_rows,) if self.n_rows > 1 else ())
        return np.array(out[:], np.float64).reshape(shape)

    def set_interference(self, idx: int, deg: float) -> int:
        """interf_theta_roscallback; returns the interferer count afterwards."""
        self._chk(self._L.bf_set_interference(self._h, int(idx), float(deg)), "bf_set_interference")
        k = self._L.bf_n_interferers(self._h)
        self.S = k + 1
        return k

    def reset(self):
        self._chk(self._L.bf_reset(self._h), "bf_reset")

    def reset_async(self, stream: int = 0):
        """Cold start enqueued on `stream` (no host synchronisation)."""
        self._chk(self._L.bf_reset_async(self._h, stream or None), "bf_reset_async")

    def kernel_timing_begin(self):
        self._chk(self._L.bf_kernel_timing_begin(self._h), "bf_kernel_timing_begin")

    def kernel_timing_end(self):
        """(mean ms per launch of the dominant kernel since begin, launches)"""
        ms, n = C.c_float(), C.c_int()
        self._chk(self._L.bf_kernel_timing_end(self._h, C.byref(ms), C.byref(n)), "bf_kernel_timing_end")
        return float(ms.value), int(n.value)

    def weights(self) -> np.ndarray:
        w = np.empty((self.N, self.M, self.S), np.complex128)
        self._chk(self._L.bf_get_weights(self._h, w.ctypes.data), "bf_get_weights")
        return w

    def process_hop(self, x: np.ndarray) -> np.ndarray:
        """x [M, H] float32 (host) -> [H] float32: one jack_callback ([n_dirs, H] with look directions, [n_dirs, R, H] or [R, H] with
        gss_out_sources / lcmv_out_beams = R > 1)."""
        x = np.ascontiguousarray(x, np.float32)
        assert x.shape == (self.M, self.H)
        ptrs = (C.c_void_p * self.M)(*[x[m].ctypes.data for m in range(self.M)])
        out = np.empty((self.n_dirs, self.n_rows, self.H), np.float32)
        self._chk(self._L.bf_process_hop(self._h, ptrs, out.ctypes.data, self.H), "bf_process_hop")
        out = out if self.n_rows > 1 else out[:, 0]
        return out[0] if self.n_dirs == 1 else out

    def process(self, x: np.ndarray, out: np.ndarray = None) -> np.ndarray:
        """Host batch. planar: x [S, M, F*H] (or [M, F*H] when S == 1); interleaved: [S, F*H, M].  -> [output streams, F*H] ([F*H] when
        there is one), output stream = stream * n_dirs + dir; with gss_out_sources / lcmv_out_beams = R > 1 the rows are an axis of their own behind it:
        [n_streams * n_dirs, R, F*H], or [R, F*H] for one beam."""
        x = np.ascontiguousarray(x, np.float32)
        n = x.size // (self.n_streams * self.M * self.H)
        y = np.empty((self.n_out, n * self.H), np.float32) if out is None else out
        assert y.dtype == np.float32 and y.size == self.n_out * n * self.H and y.flags.c_contiguous
        self._chk(self._L.bf_process_batch(self._h, x.ctypes.data, n, y.ctypes.data), "bf_process_batch")
        y = y.reshape(self.n_out, n * self.H)
        if self.n_rows > 1:
            y = y.reshape(self.n_out // self.n_rows, self.n_rows, n * self.H)
            return y[0] if y.shape[0] == 1 else y
        return y[0] if self.n_out == 1 else y

    def process_device(self, x_ptr: int, n_frames: int, y_ptr: int, spectrum_ptr: int = 0, stream: int = 0):
        self._chk(self._L.bf_process_batch_device(self._h, x_ptr, n_frames, y_ptr, spectrum_ptr or None, stream or None),
                  "bf_process_batch_device")

    def set_track_angles(self, angles):
        """Installs the candidate angles (degrees) of steering tracks: one table per angle, the one set_theta(angle) would build
        (bf_track_set_angles; host-synchronous).  An empty list drops them.  das in double, phase and phasempf with one look direction."""
        a = np.ascontiguousarray(angles, np.float64).ravel()
        ptr = a.ctypes.data_as(C.POINTER(C.c_double)) if a.size else None
        self._chk(self._L.bf_track_set_angles(self._h, ptr, int(a.size)), "bf_track_set_angles")

    def process_device_tracked(self, x_ptr: int, n_frames: int, y_ptr: int, track_ptr: int, spectrum_ptr: int = 0, stream: int = 0):
        """process_device with a look angle per frame: track_ptr -> int32 [n_streams][n_frames] on the device, frame t of stream s is
        weighted with the table of angle track[s][t]; any index outside the installed angles (-1, say) means the handle's own theta."""
        self._chk(self._L.bf_process_batch_device_tracked(self._h, x_ptr, n_frames, y_ptr, spectrum_ptr or None, track_ptr or None,
                                                          stream or None), "bf_process_batch_device_tracked")

    def set_ctrack_angles(self, angles):
        """set_track_angles for mvdr / lcmv (bf_ctrack_set_angles; host-synchronous): one table per candidate angle, shared by the look
        direction and every interferer column.  An empty list drops them."""
        a = np.ascontiguousarray(angles, np.float64).ravel()
        ptr = a.ctypes.data_as(C.POINTER(C.c_double)) if a.size else None
        self._chk(self._L.bf_ctrack_set_angles(self._h, ptr, int(a.size)), "bf_ctrack_set_angles")

    def process_device_ctracked(self, x_ptr: int, n_frames: int, y_ptr: int, track_ptr: int, n_cols: int, spectrum_ptr: int = 0, stream: int = 0):
        """process_device with an angle per frame and constraint column (mvdr / lcmv): track_ptr -> int32 [n_streams][n_frames][n_cols] on
        the device, column 0 = look direction, column c = interferer c; an index outside the installed angles (-1, say) means the
        handle's own column, and so does every column from n_cols on."""
        self._chk(self._L.bf_process_batch_device_ctracked(self._h, x_ptr, n_frames, y_ptr, spectrum_ptr or None, track_ptr or None,
                                                           int(n_cols), stream or None), "bf_process_batch_device_ctracked")

    def process_device_strided(self, x_ptr: int, n_frames: int, y_ptr: int, mic_stride: int, stream: int = 0):
        """process_device on a column range of a longer planar buffer (microphone m at x_ptr + m * mic_stride samples)."""
        self._chk(self._L.bf_process_batch_device_strided(self._h, x_ptr, n_frames, y_ptr, stream or None, mic_stride),
                  "bf_process_batch_device_strided")

    def time_device(self, x_ptr: int, n_frames: int, y_ptr: int, iters: int, stream: int = 0):
        """(mean ms per call, mean ms per launch of the dominant kernel), HIP events on `stream`."""
        ms, msk = C.c_float(), C.c_float()
        self._chk(self._L.bf_time_batch_device(self._h, x_ptr, n_frames, y_ptr, stream or None, iters, C.byref(ms),
                                               C.byref(msk)), "bf_time_batch_device")
        return float(ms.value), float(msk.value)

    def get_state(self) -> bytes:
        n = self._L.bf_state_size(self._h)
        buf = C.create_string_buffer(n)
        self._chk(self._L.bf_get_state(self._h, buf, n), "bf_get_state")
        return buf.raw

    def set_state(self, blob: bytes):
        self._chk(self._L.bf_set_state(self._h, blob, len(blob)), "bf_set_state")


def track_from_peaks_device(peak_ptr: int, map_ptr: int, n_angles: int, n_streams: int, n_blocks: int, frames_per_block: int,
                            latency_blocks: int, min_peak: float, carry_ptr: int, track_ptr: int, stream: int = 0):
    """Doa peaks [n_streams][n_blocks] (and maps, 0 = none when min_peak <= 0) -> the steering track [n_streams][n_blocks * frames_per_block]
    of their frames, on the device (bf_track_from_peaks_device): every frame of block b gets the peak of the latest block
    <= b - latency_blocks whose map value at the peak is not below min_peak, carry[s] where there is none; carry [n_streams] int32 is
    updated so that the next call continues the stream (start with -1: the handle's theta)."""
    L = load()
    rc = L.bf_track_from_peaks_device(peak_ptr or None, map_ptr or None, int(n_angles), int(n_streams), int(n_blocks),
                                      int(frames_per_block), int(latency_blocks), float(min_peak), carry_ptr or None, track_ptr or None,
                                      stream or None)
    if rc:
        raise BfError(rc, "bf_track_from_peaks_device", (L.bf_last_error(None) or b"").decode() or L.bf_strerror(rc).decode())


def doa_pick_device(map_ptr: int, angles_ptr: int, n_angles: int, n_streams: int, n_blocks: int, k: int, min_sep_deg: float,
                    rel_floor: float, picks_ptr: int, stream: int = 0):
    """Doa maps [n_streams][n_blocks][n_angles] and the grid [n_angles] float64 (degrees, on the device) -> picks
    [n_streams][n_blocks][k] int32, on the device (bf_doa_pick_device): per row controllers.pick_sources' indices, strongest first, -1 in
    the unused places."""
    L = load()
    rc = L.bf_doa_pick_device(map_ptr or None, angles_ptr or None, int(n_angles), int(n_streams), int(n_blocks), int(k),
                              float(min_sep_deg), float(rel_floor), picks_ptr or None, stream or None)
    if rc:
        raise BfError(rc, "bf_doa_pick_device", (L.bf_last_error(None) or b"").decode() or L.bf_strerror(rc).decode())


def ctrack_from_picks_device(picks_ptr: int, map_ptr: int, n_angles: int, k: int, n_streams: int, n_blocks: int, frames_per_block: int,
                             latency_blocks: int, min_peak: float, n_cols: int, carry_ptr: int, track_ptr: int, stream: int = 0):
    """Picks [n_streams][n_blocks][k] (and maps, 0 = none when min_peak <= 0) -> the column track
    [n_streams][n_blocks * frames_per_block][n_cols] of their frames, on the device (bf_ctrack_from_picks_device): controllers.sources_track
    with a DoaSources controller.  A block publishes when its first pick's map value is not below min_peak; column c of every frame of
    block b is pick c of the latest block <= b - latency_blocks that published one, carry[s][c] where there is none; carry
    [n_streams][n_cols] int32 is updated so that the next call continues the stream (start with -1: the handle's own columns)."""
    L = load()
    rc = L.bf_ctrack_from_picks_device(picks_ptr or None, map_ptr or None, int(n_angles), int(k), int(n_streams), int(n_blocks),
                                       int(frames_per_block), int(latency_blocks), float(min_peak), int(n_cols), carry_ptr or None,
                                       track_ptr or None, stream or None)
    if rc:
        raise BfError(rc, "bf_ctrack_from_picks_device", (L.bf_last_error(None) or b"").decode() or L.bf_strerror(rc).decode())


def ctrack_assign_device(picks_ptr: int, map_ptr: int, angles_ptr: int, n_angles: int, k: int, n_streams: int, n_blocks: int,
                         frames_per_block: int, latency_blocks: int, min_peak: float, gate_deg: float, min_hits: int, max_coast: int,
                         n_cols: int, state_ptr: int, track_ptr: int, active_ptr: int = 0, stream: int = 0):
    """Picks [n_streams][n_blocks][k] (maps, 0 = none when min_peak <= 0; the picker's grid [n_angles] float64 on the device) -> a column
    track [n_streams][n_blocks * frames_per_block][n_cols] in which a column is a talker, on the device (bf_ctrack_assign_device):
    controllers.assign_sources.  Per block the picks of a publishing block are matched to the live columns, nearest pair within gate_deg
    first; a column that was not heard coasts for up to max_coast blocks and is then freed, an unmatched pick is born into the lowest
    free column and counts from its min_hits-th block on.  state [n_streams][n_cols][BF_ASSIGN_STATE_INTS] int32 {idx, hits, misses,
    out} is read and updated so that the next call continues the stream (start with -1); active (0 = none)
    [n_streams][n_blocks][n_cols] int32 says which columns were heard in which block."""
    L = load()
    rc = L.bf_ctrack_assign_device(picks_ptr or None, map_ptr or None, angles_ptr or None, int(n_angles), int(k), int(n_streams),
                                   int(n_blocks), int(frames_per_block), int(latency_blocks), float(min_peak), float(gate_deg),
                                   int(min_hits), int(max_coast), int(n_cols), state_ptr or None, track_ptr or None, active_ptr or None,
                                   stream or None)
    if rc:
        raise BfError(rc, "bf_ctrack_assign_device", (L.bf_last_error(None) or b"").decode() or L.bf_strerror(rc).decode())


class Doa:
    """Direction-of-arrival maps (bf_doa_*; SRP-PHAT by default, Capon and MUSIC through set_method): per block of `frames_per_block` frames, the PHAT-weighted steered response
    power of every angle in `angles` (degrees) over the band [freq_lo, freq_hi] Hz, and the index of the best angle.  `params`
    supplies the geometry, hop and sample rate (a beamform_amd.params dict); the angle of a peak is what das takes in set_theta."""

    def __init__(self, params: dict, angles, freq_lo: float, freq_hi: float, frames_per_block: int, device: int = 0,
                 n_streams: int = 1, layout: int = BF_PLANAR, phat_floor: float = None):
        self._L = load()
        self.cfg = config_from_params(params, device, n_streams, layout)
        self.angles = np.ascontiguousarray(angles, np.float64).ravel()
        self.M, self.H = params["n_mics"], params["hop"]
        self.W, self.n_streams = int(frames_per_block), n_streams
        self._h = C.c_void_p()
        a = self.angles.ctypes.data_as(C.POINTER(C.c_double)) if self.angles.size else None
        rc = self._L.bf_doa_create(C.byref(self.cfg), a, int(self.angles.size), float(freq_lo), float(freq_hi), self.W,
                                   C.byref(self._h))
        if rc:
            raise BfError(rc, "bf_doa_create", self._L.bf_last_error(None).decode())
        if phat_floor is not None:
            self.set_phat_floor(phat_floor)

    def close(self):
        if getattr(self, "_h", None):
            self._L.bf_doa_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def _chk(self, rc, what):
        if rc:
            raise BfError(rc, what, (self._L.bf_last_error(None) or b"").decode() or self._L.bf_strerror(rc).decode())

    def set_phat_floor(self, eps: float):
        self._chk(self._L.bf_doa_set_phat_floor(self._h, float(eps)), "bf_doa_set_phat_floor")

    def set_method(self, method):
        """"srp_phat" (the default), "capon" or "music" (or the BF_DOA_* constant): the map the next process call computes.  The Capon map
        tells several sources apart where the SRP-PHAT map shows the strongest one's sidelobes (controllers.follow_sources); the MUSIC
        map does so from the noise subspace of the same covariances, and comes with the eigenvalue profile (process(x, eig=True))."""
        m = {"srp_phat": BF_DOA_SRP_PHAT, "capon": BF_DOA_CAPON, "music": BF_DOA_MUSIC}.get(method, method)
        if isinstance(m, str):
            raise ValueError(f"unknown Doa method {method!r}")
        self._chk(self._L.bf_doa_set_method(self._h, int(m)), "bf_doa_set_method")

    def set_loading(self, delta: float):
        """Capon's diagonal loading, in (0, 1] (default 1e-3)."""
        self._chk(self._L.bf_doa_set_loading(self._h, float(delta)), "bf_doa_set_loading")

    def set_sources(self, n_sources: int):
        """MUSIC's signal-subspace dimension, 1 .. n_mics - 1 (default 1); controllers.count_sources reads it off a profile."""
        self._chk(self._L.bf_doa_set_sources(self._h, int(n_sources)), "bf_doa_set_sources")

    def set_music_floor(self, mu: float):
        """MUSIC's map is mu / (mu + the noise-subspace response), mu in (0, 1] (default 1e-2): the contrast, never the order."""
        self._chk(self._L.bf_doa_set_music_floor(self._h, float(mu)), "bf_doa_set_music_floor")

    def reset(self):
        self._chk(self._L.bf_doa_reset(self._h), "bf_doa_reset")

    def process(self, x: np.ndarray, eig: bool = False):
        """Host batch, layout as Beamformer.process -> (map [n_streams, n_blocks, n_angles] float64, peak [n_streams, n_blocks] int32);
        the leading axis is dropped when n_streams == 1.  eig=True (the MUSIC method only): (map, peak, E) with the eigenvalue profile
        E [n_streams, n_blocks, n_mics] float64, descending."""
        x = np.ascontiguousarray(x, np.float32)
        n = x.size // (self.n_streams * self.M * self.H)
        nb = n // self.W if self.W else 0
        m = np.empty((self.n_streams, nb, self.angles.size), np.float64)
        p = np.empty((self.n_streams, nb), np.int32)
        if eig:
            e = np.empty((self.n_streams, nb, self.M), np.float64)
            self._chk(self._L.bf_doa_process_eig(self._h, x.ctypes.data, n, m.ctypes.data, p.ctypes.data, e.ctypes.data),
                      "bf_doa_process_eig")
            return (m[0], p[0], e[0]) if self.n_streams == 1 else (m, p, e)
        self._chk(self._L.bf_doa_process(self._h, x.ctypes.data, n, m.ctypes.data, p.ctypes.data), "bf_doa_process")
        return (m[0], p[0]) if self.n_streams == 1 else (m, p)

    def process_device(self, x_ptr: int, n_frames: int, map_ptr: int = 0, peak_ptr: int = 0, stream: int = 0, eig_ptr: int = 0):
        """Device buffers: map [n_streams][n_frames/W][n_angles] float64 and / or peak [n_streams][n_frames/W] int32; eig_ptr (the MUSIC
        method only): the eigenvalue profile [n_streams][n_frames/W][n_mics] float64."""
        if eig_ptr:
            self._chk(self._L.bf_doa_process_device_eig(self._h, x_ptr, n_frames, map_ptr or None, peak_ptr or None, eig_ptr,
                                                        stream or None), "bf_doa_process_device_eig")
            return
        self._chk(self._L.bf_doa_process_device(self._h, x_ptr, n_frames, map_ptr or None, peak_ptr or None, stream or None),
                  "bf_doa_process_device")
