"""Steering controllers: the host-side mirror of the reference's /theta publishers.

The reference closes the loop outside the node: a Python script subscribes to the node's output windows
(`jackaudio`, one message per JACK period), estimates an energy over the last `num_win` windows and publishes a new
/theta by a gradient step on that energy (scripts/energy2theta.py:62-101 and its -diff / -spec variants,
scripts/SIR2theta.py:9-26).  These classes keep that behaviour -- same gate, same window deque, same energy
estimators, same step and wrap rule -- as plain objects with one method per ROS callback, so the loop can run around a
`Beamformer` (`follow`) one period at a time, exactly as the topics would drive it.  Control plane only: the data path
stays in the HIP kernels; `beamform_amd.capi.Beamformer.stream_rms` (bf_stream_rms) is the same
`get_energy_from_list` quantity evaluated on the GPU when the windows stay resident (examples/theta_scan.cpp).

Python because the reference's controllers are Python; numpy/scipy only.
"""
from __future__ import annotations

import math
from collections import deque

import numpy as np

INVALID = -100.0   # the scripts' "no energy yet" sentinel (energy2theta.py:17)


def window_rms(win) -> float:
    """get_energy_from_list (energy2theta.py:23-27): root mean square of one output window."""
    w = np.asarray(win, dtype=np.float64)
    return math.sqrt(float(np.sum(w * w)) / len(w))


def wrap180(theta: float) -> float:
    """energy2theta.py:85-88: one wrap step, not a modulo (a step larger than 360 degrees stays out of range, as there)."""
    if theta > 180:
        return theta - 360
    if theta < -180:
        return theta + 360
    return theta


class Energy2Theta:
    """scripts/energy2theta.py: gradient ASCENT on the expected |sample| of the last `num_win` active windows.

    on_window(win) is energycallback (:62-101): windows below the VAD threshold are ignored altogether; the first
    `num_win` active windows only fill the deque; from then on every active window slides the deque, estimates the
    energy and publishes theta = past_theta + mu * (energy - past_energy), wrapped once into [-180, 180].
    The energy (get_energy_from_deque, :29-60) is the expectation of |x| under a histogram whose bin edges are chosen by
    numpy's Freedman-Diaconis rule on the FIRST evaluation and frozen afterwards (left bin edges x relative counts)."""

    def __init__(self, initial_angle: float = 0.0, num_win: int = 50, vad_threshold: float = 0.001, mu: float = 25.0):
        self.num_win, self.vad_threshold, self.mu = int(num_win), float(vad_threshold), float(mu)
        self.past_theta = float(initial_angle)      # rospy.get_param('/beamform/initial_angle') (:109-112)
        self.past_energy = INVALID
        self.windows = deque()
        self.hist_bins = None
        self.n_published = 0

    def deque_energy(self) -> float:
        data = np.abs(np.concatenate([np.asarray(w, dtype=np.float64) for w in self.windows]))
        if self.hist_bins is None:
            counts, edges = np.histogram(data, "fd")
            self.hist_bins = edges
        else:
            counts, edges = np.histogram(data, self.hist_bins)
        p = counts.astype(float) / len(data)
        return float(np.sum(edges[0:-1] * p))

    def step(self, energy: float) -> float:
        theta = wrap180(self.past_theta + self.mu * (energy - self.past_energy))
        self.past_energy, self.past_theta = energy, theta
        self.n_published += 1
        return theta

    def on_window(self, win):
        """One `jackaudio` message.  Returns the theta to publish, or None."""
        if window_rms(win) < self.vad_threshold:
            return None
        if len(self.windows) < self.num_win:
            self.windows.append(np.array(win, dtype=np.float64))
            return None
        self.windows.popleft()
        self.windows.append(np.array(win, dtype=np.float64))
        if self.past_energy == INVALID:
            self.past_energy = self.deque_energy()
        return self.step(self.deque_energy())


class Energy2ThetaDiff:
    """scripts/energy2theta-diff.py: gradient DESCENT on the RMS of (reference channel - beamformer output) over the last
    `num_win` windows (:72-103).  Unlike energy2theta the deque slides on every message; only the step is VAD-gated, and the
    energy is the plain RMS of the deque (:60)."""

    def __init__(self, initial_angle: float = 0.0, num_win: int = 50, vad_threshold: float = 0.001, mu: float = 25.0):
        self.num_win, self.vad_threshold, self.mu = int(num_win), float(vad_threshold), float(mu)
        self.past_theta = float(initial_angle)
        self.past_energy = INVALID
        self.windows = deque()

    def deque_energy(self) -> float:
        data = np.abs(np.concatenate(list(self.windows)))
        return math.sqrt(float(np.mean(data ** 2)))

    def on_windows(self, win, win_ref):
        """One synchronised (`jackaudio`, `jackaudio_ref`) pair.  Returns the theta to publish, or None."""
        d = np.asarray(win_ref, dtype=np.float64) - np.asarray(win, dtype=np.float64)
        if len(self.windows) >= self.num_win:
            self.windows.popleft()
        self.windows.append(d)
        if window_rms(d) < self.vad_threshold:
            return None
        if self.past_energy == INVALID:
            self.past_energy = self.deque_energy()
        energy = self.deque_energy()
        theta = wrap180(self.past_theta - self.mu * (energy - self.past_energy))
        self.past_energy, self.past_theta = energy, theta
        return theta


class Energy2ThetaSpec:
    """scripts/energy2theta-spec.py (:105-150): as -diff, but the deque must be full before anything else happens, the
    step is an ascent again, and the energy is one of
      'history'     (:77-94)  last window's RMS / ((last - mean of the deque's window RMSs) * 1000), mu = 10
      'spectrogram' (:55-75)  sqrt(mean of the spectrogram bins above fft_threshold) of the whole deque, mu = 5000
    A NaN energy (e.g. an empty thresholded spectrogram) is "invalid" (-100) and suppresses the step (:100-101, :134)."""

    def __init__(self, initial_angle: float = 0.0, num_win: int = 100, vad_threshold: float = 0.001, method: str = "history",
                 fs: float = 48000.0, fft_threshold: float = 0.00001):
        self.num_win, self.vad_threshold = int(num_win), float(vad_threshold)
        self.method, self.fs, self.fft_threshold = method, float(fs), float(fft_threshold)
        self.mu = 5000.0        # the module-level value; every energy evaluation overwrites it per method (:64, :82)
        self.past_theta = float(initial_angle)
        self.past_energy = INVALID
        self.windows = deque()
        self.n_seen = 0

    def deque_energy(self) -> float:
        if self.method == "spectrogram":
            from scipy import signal
            self.mu = 5000.0
            data = np.concatenate(list(self.windows))
            _, _, spec = signal.spectrogram(data, self.fs, nperseg=1024, noverlap=512, scaling="spectrum")
            sel = spec[spec > self.fft_threshold]
            with np.errstate(invalid="ignore"):
                energy = math.sqrt(np.mean(sel)) if sel.size else float("nan")
        elif self.method == "history":
            self.mu = 10.0
            alpha = 1000
            past = np.array([np.sqrt(np.mean(np.asarray(w) ** 2)) for w in self.windows])
            delta = past[-1] - np.mean(past)
            with np.errstate(divide="ignore", invalid="ignore"):
                energy = float(past[-1] / (delta * alpha))
        else:
            energy = INVALID
        return INVALID if math.isnan(energy) else energy

    def on_windows(self, win, win_ref):
        d = np.asarray(win_ref, dtype=np.float64) - np.asarray(win, dtype=np.float64)
        if self.n_seen < self.num_win:
            self.windows.append(d)
            self.n_seen += 1
            return None
        self.windows.popleft()
        self.windows.append(d)
        if window_rms(d) < self.vad_threshold:
            return None
        if self.past_energy == INVALID:
            self.past_energy = self.deque_energy()
        energy = self.deque_energy()
        if not energy > INVALID:
            return None
        theta = wrap180(self.past_theta + self.mu * (energy - self.past_energy))
        self.past_energy, self.past_theta = energy, theta
        return theta


class SIR2Theta:
    """scripts/SIR2theta.py:9-26: theta = past_theta - mu * (SIR - past_SIR) on every /SIR message; starts at theta = 1.0
    (published once at start-up, :37) with past_SIR = -100; no wrap."""

    def __init__(self, mu: float = 0.01, initial_theta: float = 1.0):
        self.mu, self.past_theta, self.past_sir = float(mu), float(initial_theta), INVALID

    def initial(self) -> float:
        return self.past_theta

    def on_sir(self, sir: float) -> float:
        theta = self.past_theta - self.mu * (float(sir) - self.past_sir)
        self.past_sir, self.past_theta = float(sir), theta
        return theta


class Vad:
    """scripts/vad.py:24-66: the two-state (silence / active) energy detector some launch set-ups run beside the node."""

    def __init__(self, tchange: float = 0.015, tvad: float = 0.02, ehist_len: int = 8, windows_passed_threshold: int = 5):
        self.tchange, self.tvad, self.limit = tchange, tvad, windows_passed_threshold
        self.ehist = np.zeros(ehist_len)
        self.i = 0
        self.enoise = 0.0
        self.passed = 0
        self.silence = False
        self.active = False

    def on_window(self, win) -> bool:
        e = float(np.absolute(np.asarray(win, dtype=np.float64)).mean())
        if (not self.silence) and e > self.enoise + self.tvad:
            self.passed = 0
            self.active = True
        else:
            self.active = False
            self.passed += 1
        mean = float(np.absolute(self.ehist).mean())
        if self.silence and e > mean + self.tchange:
            self.silence = False
            self.enoise = mean
            self.ehist = np.ones(len(self.ehist)) * mean
        elif (not self.silence) and (e < mean - self.tchange or self.passed > self.limit):
            self.passed = 0
            self.silence = True
            self.ehist = np.ones(len(self.ehist)) * self.enoise
        else:
            self.ehist[self.i] = e
            self.i = (self.i + 1) % len(self.ehist)
        return self.active


class JackRef:
    """beamform/src/jack_ref.cpp:19-30 + util.h:353-379 (do_overlap_bymic): the reference channel of the two-topic controllers
    -- one microphone "in the same delayed manner as the rest of the frequency-domain beamformers", i.e. through the WOLA
    framing with NO processing in between: frame t = [hop t-1 | hop t] times the sqrt-Hann window (util.h:235, in double),
    stored as float, times the window again (jack_ref.cpp:26-29, float x double -> float), overlap-added
    (util.h:301-302).  sqrt-Hann^2 at 50 % overlap sums to one, so the output is the input delayed by ONE hop (to float
    rounding): sample-aligned with the beamformer output that energy2theta-diff.py:74 subtracts from it."""

    def __init__(self, hop: int = 512):
        self.H = int(hop)
        n = np.arange(2 * self.H, dtype=np.float64)
        self.win = np.sqrt(0.5 - 0.5 * np.cos(2.0 * np.pi * n / (2 * self.H)))  # util.h:201-211
        self.prev_hop = np.zeros(self.H, np.float32)   # ring pre-filled with one hop of zeros (util.h:272-277)
        self.tail = np.zeros(self.H, np.float32)       # out_buff calloc'ed (util.h:285-286)

    def process_hop(self, s) -> np.ndarray:
        s = np.asarray(s, np.float32)
        frame = np.concatenate([self.prev_hop, s]).astype(np.float64) * self.win   # overlap_and_add_prepare_input
        o = frame.astype(np.float32)                                              # out[j] = real(x[j])
        o = (o.astype(np.float64) * self.win).astype(np.float32)                  # out[j] *= hann_win[j]
        y = self.tail + o[:self.H]                                                # float + float (util.h:301-302)
        self.tail, self.prev_hop = o[self.H:].copy(), s.copy()
        return y


def follow(node, x: np.ndarray, controller, ref_channel: int = 0):
    """The closed loop of the reference, one JACK period at a time: node.process_hop -> controller -> node.set_theta.

    node: anything with process_hop([M, hop]) -> [hop], set_theta(deg) and an attribute H (beamform_amd.capi.Beamformer;
    the tests also drive the oracle node through it).  x: [M, F*hop] float32.  For the two-topic controllers
    (-diff / -spec) the reference channel is microphone `ref_channel` through the jackaudio_ref node (JackRef above): the same
    one-hop WOLA latency as the beamformer output, so the difference the controller forms is sample-aligned.
    Returns (y [F*hop], thetas: list of (hop index, theta) published)."""
    H = node.H
    F = x.shape[1] // H
    ys, published = [], []
    ref = JackRef(H) if hasattr(controller, "on_windows") else None
    for t in range(F):
        seg = np.ascontiguousarray(x[:, t * H:(t + 1) * H])
        y = node.process_hop(seg)
        if isinstance(y, tuple):
            y = y[0]
        ys.append(np.array(y, copy=True))
        if hasattr(controller, "on_windows"):
            theta = controller.on_windows(y, ref.process_hop(seg[ref_channel]))
        else:
            theta = controller.on_window(y)
        if theta is not None:
            node.set_theta(theta)
            published.append((t, theta))
    return np.concatenate(ys), published


class DoaTheta:
    """A /theta publisher driven by a direction-of-arrival map (beamform_amd.capi.Doa, bf_doa_*): on_map(row) returns the angle
    of the block's peak, or None when the map value there is below `min_peak` (nothing to steer to)."""

    def __init__(self, angles, min_peak: float = 0.0):
        self.angles = np.asarray(angles, dtype=np.float64).ravel()
        self.min_peak = float(min_peak)

    def on_map(self, row):
        row = np.asarray(row, dtype=np.float64)
        d = int(np.argmax(row))  # the lowest index on ties, as bf_doa's peak
        if row[d] < self.min_peak:
            return None
        return float(self.angles[d])


def follow_doa(node, doa, x: np.ndarray, frames_per_block: int, controller):
    """The closed loop with a localiser in place of the gradient scripts, one block of `frames_per_block` JACK periods at a time:
    doa.process(block) -> controller.on_map(map row) -> node.set_theta, the node processing the same block with the angle the
    PREVIOUS block published (one block of latency, as an external localiser has).

    node: process(x [M, n*hop]) -> [n*hop], set_theta(deg), attribute H (beamform_amd.capi.Beamformer).  doa: beamform_amd.capi.Doa
    on the same geometry, one stream, W = frames_per_block.  x: [M, F*hop] float32, F a multiple of frames_per_block.
    Returns (y [F*hop], published: list of (block index, theta)), the shape of follow()'s result."""
    H, W = node.H, int(frames_per_block)
    F = x.shape[1] // H
    ys, published = [], []
    for b in range(F // W):
        seg = np.ascontiguousarray(x[:, b * W * H:(b + 1) * W * H])
        m, _ = doa.process(seg)
        y = node.process(seg)
        ys.append(np.array(y, copy=True))
        theta = controller.on_map(m[0])
        if theta is not None:
            node.set_theta(theta)
            published.append((b, theta))
    return np.concatenate(ys), published


def follow_doa_device(node, doa, x: np.ndarray, frames_per_block: int, min_peak: float = 0.0):
    """follow_doa with DoaTheta(doa.angles, min_peak) for a whole recording in three enqueues on one stream and no host synchronisation
    in between: doa.process_device (maps and peaks of every block), track_from_peaks_device (latency 1, carry -1: block b is steered
    by what the latest block before it published, block 0 and everything in front of the first publication by the node's own theta)
    and node.process_device_tracked.  Peaks and maps come back once, at the end, for the list of publications.

    node: beamform_amd.capi.Beamformer (das in double, phase or phasempf, one stream); its track angles are replaced by doa.angles and
    its theta is left at the last published angle, as follow_doa leaves it.  doa: beamform_amd.capi.Doa on the same geometry, one
    stream, W = frames_per_block.  x: [M, F*hop] float32 on the host, F a multiple of frames_per_block.
    Returns (y [F*hop], published: list of (block index, theta))."""
    import torch
    from .capi import track_from_peaks_device
    H, W = node.H, int(frames_per_block)
    F = x.shape[1] // H
    nb, A = F // W, int(doa.angles.size)
    node.set_track_angles(doa.angles)
    st = torch.cuda.current_stream().cuda_stream
    xd = torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()
    maps = torch.empty((nb, A), dtype=torch.float64, device="cuda")
    peaks = torch.empty((nb,), dtype=torch.int32, device="cuda")
    carry = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    track = torch.empty((nb * W,), dtype=torch.int32, device="cuda")
    yd = torch.empty((nb * W * H,), dtype=torch.float32, device="cuda")
    doa.process_device(xd.data_ptr(), nb * W, maps.data_ptr(), peaks.data_ptr(), st)
    track_from_peaks_device(peaks.data_ptr(), maps.data_ptr(), A, 1, nb, W, 1, min_peak, carry.data_ptr(), track.data_ptr(), st)
    node.process_device_tracked(xd.data_ptr(), nb * W, yd.data_ptr(), track.data_ptr(), 0, st)
    y, pk, mp = yd.cpu().numpy(), peaks.cpu().numpy(), maps.cpu().numpy()
    published = [(b, float(doa.angles[pk[b]])) for b in range(nb) if not mp[b, pk[b]] < min_peak]
    if published:
        node.set_theta(published[-1][1])
    return y, published


def pick_sources(row, angles, k: int, min_sep_deg: float, rel_floor: float = 0.0):
    """Greedy peak picking on one map row (a Capon map tells several sources apart: capi.Doa.set_method("capon")): repeatedly the
    largest remaining value, the lowest index on ties; every angle whose circular distance to a picked angle is below `min_sep_deg`
    is suppressed.  Stops after `k` picks, when nothing remains, or when the value is below `rel_floor` x the row's maximum.
    Returns the picked indices, strongest first."""
    row = np.asarray(row, dtype=np.float64).ravel()
    ang = np.asarray(angles, dtype=np.float64).ravel()
    if row.size == 0:
        return []
    floor = float(rel_floor) * float(np.max(row))
    free = np.ones(row.size, bool)
    picks = []
    while len(picks) < int(k) and free.any():
        d = int(np.argmax(np.where(free, row, -np.inf)))  # the lowest index on ties
        if row[d] < floor:
            break
        picks.append(d)
        free &= np.abs((ang - ang[d] + 180.0) % 360.0 - 180.0) >= float(min_sep_deg)
        free[d] = False
    return picks


def count_sources(E_row, rel: float = 0.02, n_max: int = None) -> int:
    """The number of sources one eigenvalue profile shows (capi.Doa.set_method("music"), process(x, eig=True): a row of E, descending):
    the leading entries with E[i] >= rel * E[0], at least 1 and at most `n_max` (default: len - 1, the most MUSIC can separate).
    The count is the evidence for pick_sources' k and Doa.set_sources; rel = 0.02 keeps a second source 17 dB under the first and
    drops the sensor noise of the project's scenes (EXPERIMENTS.md has the profiles it was read from)."""
    e = np.asarray(E_row, dtype=np.float64).ravel()
    if n_max is None:
        n_max = e.size - 1
    n = 0
    while n < e.size and e[n] >= float(rel) * e[0]:
        n += 1
    return max(1, min(n, int(n_max)))


class DoaSources:
    """A publisher of a look direction and its interferers from one map row: on_map(row) returns (theta, [interferer angles]) --
    pick_sources' strongest pick and the rest in order -- or None when the strongest value is below `min_peak`."""

    def __init__(self, angles, k: int, min_sep_deg: float, rel_floor: float = 0.0, min_peak: float = 0.0):
        self.angles = np.asarray(angles, dtype=np.float64).ravel()
        self.k, self.min_sep_deg = int(k), float(min_sep_deg)
        self.rel_floor, self.min_peak = float(rel_floor), float(min_peak)

    def on_map(self, row):
        row = np.asarray(row, dtype=np.float64).ravel()
        picks = pick_sources(row, self.angles, self.k, self.min_sep_deg, self.rel_floor)
        if not picks or row[picks[0]] < self.min_peak:
            return None
        return float(self.angles[picks[0]]), [float(self.angles[d]) for d in picks[1:]]


def follow_sources(node, doa, x: np.ndarray, frames_per_block: int, controller):
    """follow_doa's loop for the nodes that take more than one angle (lcmv, gss), one stream and one block of latency: after block b
    has been processed, a publication (theta, interferers) of controller.on_map is applied as node.set_theta(theta), then
    node.set_interference(i + 1, angle_i) for each interferer in order.  The loop never removes an interferer itself:
    bf_set_interference's own rules (update, append, merge within interf_angle_threshold) do what they do.

    node: process(x [M, n*hop]) -> [n*hop], set_theta(deg), set_interference(id, deg), attribute H.  doa: beamform_amd.capi.Doa on the
    same geometry, one stream, W = frames_per_block (the Capon method for more than one source).  x: [M, F*hop] float32.
    Returns (y [F*hop], published: list of (block index, theta, tuple of interferer angles))."""
    H, W = node.H, int(frames_per_block)
    F = x.shape[1] // H
    ys, published = [], []
    for b in range(F // W):
        seg = np.ascontiguousarray(x[:, b * W * H:(b + 1) * W * H])
        m, _ = doa.process(seg)
        y = node.process(seg)
        if isinstance(y, tuple):
            y = y[0]
        ys.append(np.array(y, copy=True))
        pub = controller.on_map(m[0])
        if pub is not None:
            theta, interf = pub
            node.set_theta(theta)
            for i, a in enumerate(interf):
                node.set_interference(i + 1, a)
            published.append((b, theta, tuple(interf)))
    return np.concatenate(ys), published


def sources_track(maps, controller, frames_per_block: int, n_cols: int, latency_blocks: int = 1):
    """follow_sources' schedule as a column track (bf_process_batch_device_ctracked), pure numpy.  maps: [nb, n_angles], one row per
    block.  Row by row, controller.on_map(row) may publish (theta, interferers); a publication of block b sets column 0 to theta and
    columns 1 ... to the interferers in order for the frames of block b + latency_blocks and later (latency_blocks = 1: "from the next
    block on", as follow_sources applies it).  A column the publication does not mention keeps its last index, interferers beyond
    n_cols - 1 are dropped, and before the first publication every column is -1 (the node's own angles).  Angles are mapped to their
    indices in controller.angles.
    Returns (track [nb * frames_per_block, n_cols] int32, published: list of (block index, theta, tuple of interferer angles))."""
    maps = np.asarray(maps, dtype=np.float64)
    if maps.ndim != 2:
        raise ValueError("maps must be [n_blocks, n_angles]")
    nb, W, n_cols, lat = maps.shape[0], int(frames_per_block), int(n_cols), int(latency_blocks)
    if W < 1 or n_cols < 1 or lat < 0:
        raise ValueError("frames_per_block >= 1, n_cols >= 1, latency_blocks >= 0")
    grid = np.asarray(controller.angles, dtype=np.float64).ravel()

    def index_of(angle):
        hit = np.flatnonzero(grid == float(angle))
        if hit.size == 0:
            raise ValueError(f"published angle {angle!r} is not one of controller.angles")
        return int(hit[0])

    state = np.full((nb + 1, n_cols), -1, np.int32)  # state[b]: the indices in force once blocks 0 .. b-1 have published
    published = []
    for b in range(nb):
        state[b + 1] = state[b]
        pub = controller.on_map(maps[b])
        if pub is None:
            continue
        theta, interf = pub
        state[b + 1, 0] = index_of(theta)
        for i, a in enumerate(list(interf)[:n_cols - 1]):
            state[b + 1, i + 1] = index_of(a)
        published.append((b, float(theta), tuple(float(a) for a in interf)))
    track = np.empty((nb * W, n_cols), np.int32)
    for b in range(nb):
        track[b * W:(b + 1) * W] = state[max(0, b - lat + 1)]
    return track, published


def follow_sources_tracked(node, doa, x: np.ndarray, frames_per_block: int, controller):
    """follow_sources for a whole recording in one pass: node.set_ctrack_angles(doa.angles), ONE doa.process_device over the recording,
    the maps to the host once, sources_track (one block of latency), ONE column-tracked batch -- instead of a doa.process, a
    node.process and up to K + 1 table rebuilds per block.

    The one difference from follow_sources: the interferer count is the node's, fixed for the batch.  A publication with more
    interferers than the node has appends none (the extra ones are dropped), and bf_set_interference's merge rule never runs inside
    the batch.

    node: beamform_amd.capi.Beamformer (mvdr or lcmv, one stream); its track angles are replaced by doa.angles, and its theta and
    interferers are left at the last publication, as follow_sources leaves them.  doa: beamform_amd.capi.Doa on the same geometry,
    one stream, W = frames_per_block, angles = controller.angles.  x: [M, F*hop] float32 on the host, F a multiple of frames_per_block.
    Returns (y [F*hop] -- [R, F*hop] when the node has lcmv_out_beams = R > 1: row r follows column r of the track --, published: list of
    (block index, theta, tuple of interferer angles))."""
    import torch
    H, W = node.H, int(frames_per_block)
    F = x.shape[1] // H
    nb, A, n_cols = F // W, int(doa.angles.size), int(node.S)
    node.set_ctrack_angles(doa.angles)
    st = torch.cuda.current_stream().cuda_stream
    xd = torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()
    maps = torch.empty((nb, A), dtype=torch.float64, device="cuda")
    R = int(getattr(node, "n_out", 1))  # lcmv_out_beams: a row per beam
    yd = torch.empty((R, nb * W * H) if R > 1 else (nb * W * H,), dtype=torch.float32, device="cuda")
    doa.process_device(xd.data_ptr(), nb * W, maps.data_ptr(), 0, st)
    track, published = sources_track(maps.cpu().numpy(), controller, W, n_cols, 1)
    td = torch.from_numpy(track).cuda()
    node.process_device_ctracked(xd.data_ptr(), nb * W, yd.data_ptr(), td.data_ptr(), n_cols, 0, st)
    y = yd.cpu().numpy()
    last = {}  # column -> the angle it was last published with
    for _, theta, interf in published:
        last[0] = theta
        for i, a in enumerate(interf[:n_cols - 1]):
            last[i + 1] = a
    if 0 in last:
        node.set_theta(last[0])
    for c in sorted(k for k in last if k > 0):
        node.set_interference(c, last[c])
    return y, published


def follow_sources_device(node, doa, x: np.ndarray, frames_per_block: int, k: int, min_sep_deg: float, rel_floor: float = 0.0,
                          min_peak: float = 0.0):
    """follow_sources_tracked with DoaSources(doa.angles, k, min_sep_deg, rel_floor, min_peak) as four enqueues on one stream, with
    nothing copied or synchronised in between: doa.process_device (the map of every block), doa_pick_device (pick_sources on the
    device), ctrack_from_picks_device (sources_track: latency 1, carry -1, n_cols = node.S) and node.process_device_ctracked.  Picks and
    maps come back once, at the end, for the list of publications.

    The track holds the picks themselves, so doa.angles should not list an angle twice (sources_track names the first of equal
    angles; with min_sep_deg > 0 a duplicate is never picked anyway).

    node, doa, x: as follow_sources_tracked takes them; the node is left at the last publication in the same way.
    Returns (y [F*hop] -- [R, F*hop] when the node has lcmv_out_beams = R > 1 --, published: list of (block index, theta, tuple of
    interferer angles))."""
    import torch
    from .capi import ctrack_from_picks_device, doa_pick_device
    H, W, k = node.H, int(frames_per_block), int(k)
    F = x.shape[1] // H
    nb, A, n_cols = F // W, int(doa.angles.size), int(node.S)
    node.set_ctrack_angles(doa.angles)
    st = torch.cuda.current_stream().cuda_stream
    xd = torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()
    ad = torch.from_numpy(np.ascontiguousarray(doa.angles, np.float64)).cuda()
    maps = torch.empty((nb, A), dtype=torch.float64, device="cuda")
    picks = torch.empty((nb, k), dtype=torch.int32, device="cuda")
    carry = torch.full((n_cols,), -1, dtype=torch.int32, device="cuda")
    track = torch.empty((nb * W, n_cols), dtype=torch.int32, device="cuda")
    R = int(getattr(node, "n_out", 1))  # lcmv_out_beams: a row per beam
    yd = torch.empty((R, nb * W * H) if R > 1 else (nb * W * H,), dtype=torch.float32, device="cuda")
    doa.process_device(xd.data_ptr(), nb * W, maps.data_ptr(), 0, st)
    doa_pick_device(maps.data_ptr(), ad.data_ptr(), A, 1, nb, k, min_sep_deg, rel_floor, picks.data_ptr(), st)
    ctrack_from_picks_device(picks.data_ptr(), maps.data_ptr(), A, k, 1, nb, W, 1, min_peak, n_cols, carry.data_ptr(), track.data_ptr(), st)
    node.process_device_ctracked(xd.data_ptr(), nb * W, yd.data_ptr(), track.data_ptr(), n_cols, 0, st)
    y, pk, mp = yd.cpu().numpy(), picks.cpu().numpy(), maps.cpu().numpy()
    published, last = [], {}  # last: column -> the angle it was last published with
    for b in range(nb):
        p0 = int(pk[b, 0])
        if not 0 <= p0 < A or mp[b, p0] < min_peak:
            continue
        rest = [int(d) for d in pk[b, 1:] if 0 <= d < A]
        published.append((b, float(doa.angles[p0]), tuple(float(doa.angles[d]) for d in rest)))
        for c, d in enumerate([p0] + rest[:n_cols - 1]):
            last[c] = float(doa.angles[d])
    if 0 in last:
        node.set_theta(last[0])
    for c in sorted(c for c in last if c > 0):
        node.set_interference(c, last[c])
    return y, published


def assign_sources(picks, maps, angles, frames_per_block: int, latency_blocks: int, min_peak: float, gate_deg: float, min_hits: int,
                   max_coast: int, n_cols: int, state=None):
    """The host counterpart of ctrack_assign_device (bf_ctrack_assign_device, include/bfcore.h), as sources_track is of the older
    builder: a column track in which a column is a talker, not a loudness rank.  picks: [S, nb, k] indices into `angles` (what
    doa_pick_device or pick_sources gives, -1 in the unused places); maps: [S, nb, A] or None (then every block with a valid first pick
    publishes); state: [S, n_cols, 4] int32 {idx, hits, misses, out} per column, None = -1 everywhere, a cold start.

    Block by block: a publishing block's valid picks are its candidates.  The closest (live column, candidate) pair within gate_deg is
    matched first (ties: the lowest column, then the lowest pick), then the next, until none is left; a matched column moves to its pick.
    A column that was not heard is freed at once while it has fewer than min_hits hits, otherwise it coasts and is freed after more than
    max_coast silent blocks.  An unmatched candidate is born into the lowest free column.  `out` of a column follows it while it is
    live and has min_hits hits, and stays where it was otherwise; the frames of block b get `out` as it stood after block
    b - latency_blocks (the incoming `out` in front of that).
    Returns (track [S, nb * frames_per_block, n_cols] int32, active [S, nb, n_cols] int32 -- heard in that block and confirmed --,
    state [S, n_cols, 4] int32 after the last block)."""
    picks = np.asarray(picks)
    if picks.ndim != 3:
        raise ValueError("picks must be [n_streams, n_blocks, k]")
    S, nb, k = picks.shape
    ang = np.asarray(angles, dtype=np.float64).ravel()
    A, W, lat, n_cols, cap = ang.size, int(frames_per_block), int(latency_blocks), int(n_cols), 1 << 30
    if W < 1 or n_cols < 1 or lat < 0 or int(min_hits) < 1 or int(max_coast) < 0 or not (np.isfinite(gate_deg) and gate_deg >= 0):
        raise ValueError("frames_per_block, n_cols, min_hits >= 1; latency_blocks, max_coast >= 0; gate_deg finite and >= 0")
    st = np.full((S, n_cols, 4), -1, np.int32) if state is None else np.array(state, dtype=np.int32).reshape(S, n_cols, 4)
    track = np.empty((S, nb * W, n_cols), np.int32)
    active = np.zeros((S, nb, n_cols), np.int32)
    for s in range(S):
        idx, hits, misses, out = ([int(v) for v in st[s, :, i]] for i in range(4))
        outs = [list(out)]  # outs[b]: `out` once blocks 0 .. b-1 have had their say
        for b in range(nb):
            row = [int(p) for p in picks[s, b]]
            cand = []
            if 0 <= row[0] < A and (maps is None or not (maps[s][b][row[0]] < min_peak)):
                cand = [p for p in row if 0 <= p < A]
            live = [c for c in range(n_cols) if 0 <= idx[c] < A]
            heard = set()
            if live and cand:
                with np.errstate(invalid="ignore"):
                    d = np.abs((ang[[idx[c] for c in live]][:, None] - ang[cand][None, :] + 180.0) % 360.0 - 180.0)
                    d = np.where(d <= gate_deg, d, np.inf)  # a NaN is not within the gate
                while np.isfinite(d).any():
                    i, j = np.unravel_index(int(np.argmin(d)), d.shape)  # the first of equal minima: the lowest column, then the lowest pick
                    c = live[i]
                    idx[c], hits[c], misses[c] = cand[j], min(hits[c] + 1, cap), 0
                    heard.add(c)
                    cand[j] = None
                    d[i, :] = np.inf
                    d[:, j] = np.inf
            for c in live:
                if c in heard:
                    continue
                if hits[c] < min_hits:
                    idx[c] = -1
                else:
                    misses[c] = min(misses[c] + 1, cap)
                    if misses[c] > max_coast:
                        idx[c] = -1
            for p in cand:
                free = [c for c in range(n_cols) if not 0 <= idx[c] < A]
                if p is None or not free:
                    continue
                c = free[0]
                idx[c], hits[c], misses[c] = p, 1, 0
                heard.add(c)
            for c in range(n_cols):
                if 0 <= idx[c] < A and hits[c] >= min_hits:
                    out[c] = idx[c]
                    active[s, b, c] = int(c in heard)
            outs.append(list(out))
        for b in range(nb):
            track[s, b * W:(b + 1) * W] = outs[max(0, b - lat + 1)]
        st[s] = np.array([idx, hits, misses, out], np.int64).astype(np.int32).T
    return track, active, st


def follow_talkers_device(node, doa, x: np.ndarray, frames_per_block: int, k: int, min_sep_deg: float, rel_floor: float = 0.0,
                          min_peak: float = 0.0, gate_deg: float = 20.0, min_hits: int = 2, max_coast: int = 8):
    """follow_sources_device with talker identities: the same four enqueues on one stream with nothing copied or synchronised in
    between, ctrack_assign_device in the third place (assign_sources: state -1, latency 1, n_cols = node.S).  Column c of the track --
    column 0 the look direction, row c of an lcmv_out_beams node's output -- is one talker: it follows the pick nearest to where that
    talker was last heard, holds through up to max_coast silent blocks and beyond (a freed column keeps its last angle until a new
    talker is born into it), and another talker becoming the loudest does not move it.

    node, doa, x: as follow_sources_device takes them.  The node is left at the last `out` of every column that has one: set_theta for
    column 0, set_interference(c, ...) for the others.
    Returns (y [F*hop] -- [R, F*hop] when the node has lcmv_out_beams = R > 1 --, columns [nb, n_cols] float64: the angle of every
    column after each block, NaN while it has none --, active [nb, n_cols] int32: the column's talker was heard in that block)."""
    import torch
    from .capi import BF_ASSIGN_STATE_INTS, ctrack_assign_device, doa_pick_device
    H, W, k = node.H, int(frames_per_block), int(k)
    F = x.shape[1] // H
    nb, A, n_cols = F // W, int(doa.angles.size), int(node.S)
    node.set_ctrack_angles(doa.angles)
    st = torch.cuda.current_stream().cuda_stream
    xd = torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()
    ad = torch.from_numpy(np.ascontiguousarray(doa.angles, np.float64)).cuda()
    maps = torch.empty((nb, A), dtype=torch.float64, device="cuda")
    picks = torch.empty((nb, k), dtype=torch.int32, device="cuda")
    state = torch.full((n_cols, BF_ASSIGN_STATE_INTS), -1, dtype=torch.int32, device="cuda")
    track = torch.empty((nb * W, n_cols), dtype=torch.int32, device="cuda")
    active = torch.empty((nb, n_cols), dtype=torch.int32, device="cuda")
    R = int(getattr(node, "n_out", 1))  # lcmv_out_beams: a row per beam
    yd = torch.empty((R, nb * W * H) if R > 1 else (nb * W * H,), dtype=torch.float32, device="cuda")
    doa.process_device(xd.data_ptr(), nb * W, maps.data_ptr(), 0, st)
    doa_pick_device(maps.data_ptr(), ad.data_ptr(), A, 1, nb, k, min_sep_deg, rel_floor, picks.data_ptr(), st)
    ctrack_assign_device(picks.data_ptr(), maps.data_ptr(), ad.data_ptr(), A, k, 1, nb, W, 1, min_peak, gate_deg, min_hits, max_coast,
                         n_cols, state.data_ptr(), track.data_ptr(), active.data_ptr(), st)
    node.process_device_ctracked(xd.data_ptr(), nb * W, yd.data_ptr(), track.data_ptr(), n_cols, 0, st)
    y, trk, act, last = yd.cpu().numpy(), track.cpu().numpy(), active.cpu().numpy(), state.cpu().numpy()[:, 3]
    # with one block of latency the frames of block b + 1 hold `out` after block b; the state holds it after the last block
    outs = np.concatenate([trk.reshape(nb, W, n_cols)[1:, 0], last[None]]) if nb else np.empty((0, n_cols), np.int32)
    grid = np.asarray(doa.angles, np.float64)
    columns = np.where(outs >= 0, grid[np.clip(outs, 0, A - 1)], np.nan)
    for c in range(n_cols):
        if 0 <= last[c] < A:
            if c == 0:
                node.set_theta(float(grid[last[c]]))
            else:
                node.set_interference(c, float(grid[last[c]]))
    return y, columns, act
