"""The launch arithmetic of the chain as the launchers carried it before csrc/chain_geom.hpp existed, restated in plain Python from those
launchers (launch_stft / launch_istft / launch_smooth of stft_istft.hip, launch_stft_bins_fused / launch_bins_end of mask_kernels.hip,
launch_mvdr_lcmv of cov_kernels.hip, launch_gss / launch_gsc_nlms of gsc_gss_kernels.hip) and from BinPipelineImpl::init's band scan --
the independent side of tests/test_chain_geom_cpu.py.  Integers only; `//` on non-negative values is C's division.

Two things differ from those launchers on purpose, and only these: a forced mvdr tile is held to 512 frames, and `fits` says whether every
value a launcher narrowed fits what it was narrowed to."""
INT_MAX, GX_MAX, GY_MAX = 2**31 - 1, 2**31 - 1, 65535
DAS, MVDR, LCMV, GSS, PHASE, PHASEMPF, MCRA, GSC = range(8)                     # bf_algo
K_STFT, K_STFT_SMALL, K_STFT_WAVE2048, K_STFT_GENERIC, K_FUSED_W64, K_FUSED_SMALL, K_FUSED_SPLIT = range(7)          # ChainFront
B_FUSED_TAIL, B_POINTWISE, B_MPF_MASK, B_MCRA, B_GSC_ALIGN, B_MVDR_FAST, B_COV2D, B_MVDR_LCMV, B_GSS, B_GSS_LANE = range(10)  # ChainBins
I_NONE, I_W64, I_F32, I_SMALL, I_SPLIT, I_GENERIC = range(6)                    # ChainIstft
T_NONE, T_SMOOTH4, T_SMOOTH, T_NLMS, T_NLMS_PAR, T_NLMS_MW = range(6)           # ChainTail
Z_NONE, Z_F64, Z_F32 = range(3)                                                 # ChainZero


def cdiv(a, b):
    return (a + b - 1) // b


def freqs(N, sr):
    """geometry.hpp frequency_vector (quirk Q1)."""
    f = [0.0] * N
    for k in range(1, N // 2):
        f[k] = (float(k) / float(N)) * sr
        f[N - k] = -(float(k) / float(N)) * sr
    f[N // 2 - 1] = sr / 2
    return f


def band(N, sr, fmin, fmax, algo):
    """BinPipelineImpl::init's scan (skip_lo / skip_hi, band_yh_lo / band_yh_hi) and launch_mvdr_lcmv's (FastPlan's band part), each as
    it stood: two scans over the same frequency table."""
    NQ = N // 2 + 2
    cov, band_node = algo in (MVDR, LCMV), algo in (MVDR, LCMV, GSS)
    out = dict(skip_lo=N, skip_hi=0, yh_lo=0, yh_hi=NQ - 1, q_lo=0, n_main=0, n_extra=0, extra_q0=0, extra_q1=0, solve0=0, nb=0, ok=1)
    if not band_node:
        return out
    f = freqs(N, sr)
    inb = lambda q: fmin <= abs(f[q]) <= fmax
    klo, khi = N, 0
    for q in range(1, NQ):
        if inb(q):
            klo, khi = min(klo, q), q
    if khi < N // 2 - 2:
        out.update(skip_lo=khi, skip_hi=N - khi)
    if cov and khi < N // 2 - 1 and klo <= khi:
        out.update(yh_lo=klo, yh_hi=khi)
    elif cov and klo > khi:
        out.update(yh_lo=1, yh_hi=0)
    q_lo = 1
    while q_lo < N // 2 and not inb(q_lo):
        q_lo += 1
    n_main = 0
    while q_lo + n_main < N // 2 and inb(q_lo + n_main):
        n_main += 1
    assert not any(inb(q) for q in range(q_lo + n_main, N // 2))
    extra = [q for q in (N // 2, N // 2 + 1) if inb(q)]
    out.update(q_lo=q_lo, n_main=n_main, n_extra=len(extra), extra_q0=(extra + [0, 0])[0], extra_q1=(extra + [0, 0])[1],
               solve0=int(algo == LCMV and inb(0)), nb=1 + n_main + len(extra))
    return out


def geom(s, p, b):
    """s: the shape (ChainShape's names), p: the plan (chain_plan_util.PLAN's names + rows, postfilter), b: band().  Returns (fits, fields):
    fields holds what the batch's launchers computed, by the names of tests/test_chain_geom_cpu.py's GEOM; everything else stays 0."""
    N, M, F, S, cus = s["n_fft"], s["n_mics"], s["n_frames"], s["n_streams"], s["n_cus"]
    NQ, hop = N // 2 + 2, N // 2
    So = S * (M if s["algo"] == GSC else s["n_dirs"])
    rows = p["rows"]
    Si = So * rows
    ints, gxs, gys = [So], [], []          # values narrowed to int / grid.x / grid.y
    g = {}

    def gx(name, v):
        g[name] = v
        gxs.append(v)

    if p["fused"]:
        fpr = 1 if N == 1024 else (2 if p["mp"] == 4 else 1) if N == 2048 else (4 if p["mp"] == 4 else 2) * (1024 // N)
        rps = cdiv(F, fpr)
        total = rps * S
        blocks = max(1, min(total, cus))
        rpb = cdiv(total, blocks)
        g.update(fpr=fpr, rps=rps, total=total, rpb=rpb)
        gx("fused_grid", cdiv(total, rpb))
        gx("tail_blocks", cdiv(So * F * 2, 256))
    else:
        np_ = ((1 if s["algo"] == MCRA else M) + 1) // 2
        front = p["front"]
        if front == K_STFT:
            slots = cus * 8
            L = min(256, max(1, cdiv(S * F * np_, slots)))
            blocks = min(cdiv(S * cdiv(F, L) * np_, 8), cus * 4)
        elif front == K_STFT_SMALL:
            kG = 1024 // N
            L = cdiv(cdiv(S * F * np_, cus * 8 * 2), kG) * kG
            L = max(kG, min(256, L))
            blocks = min(cdiv(S * cdiv(F, L) * np_, 8), cus * 4)
        elif front == K_STFT_WAVE2048:
            L = max(1, min(256, cdiv(S * F * np_, cus * 4 * 2)))
            blocks = min(cdiv(S * cdiv(F, L) * np_, 4), cus * 4)
        else:
            L = 1
            blocks = max(1, min(S * F * np_, cus * 8))
        g["run_len"] = L
        gx("stft_blocks", blocks)

    bins = p["bins"]
    if bins in (B_POINTWISE, B_MPF_MASK, B_GSC_ALIGN):
        gx("ew_blocks", cdiv(So * F * NQ, 256))
    elif bins == B_MCRA:
        ints.append(So * NQ)
        gx("lane_blocks", cdiv(So * NQ, 64))
    elif bins in (B_MVDR_LCMV, B_COV2D):
        tile = min(64, F)
        tps = cdiv(F, tile)
        ints += [tps, tps * So]
        g.update(tile=tile, tps=tps)
        if bins == B_MVDR_LCMV:
            gx("gx", tps * So)
            g["gy"] = cdiv(NQ, 256 // p["mp"])
            gys.append(g["gy"])
        else:
            gx("cov2d_grid", cdiv(tps * So, 8) * 8 * cdiv(NQ, 16))
    elif bins == B_MVDR_FAST:
        nb = b["nb"]
        km = 2 if rows > 1 and p["km"] == 1 else p["km"]
        mp = p["mp"]
        wpc = 16 if mp == 2 else (9 if km <= 2 else 8) if mp == 4 else (6 if km == 1 else 4) if mp == 6 else 4
        slots = cus * wpc
        best_t, best_c = 1, 1e300
        for t in range(1, min(512, F) + 1):
            tiles = cdiv(F, t)
            waves = So * cdiv(tiles * nb, 64)
            c = float(cdiv(waves, slots)) * float(t + s["past_windows"] + 2)
            if c <= best_c:
                best_c, best_t = c, t
        if s["mvdr_tile"] > 0:
            best_t = min(s["mvdr_tile"], F, 512)          # the clamp: the one intended change
        tiles = cdiv(F, best_t)
        wps = cdiv(tiles * nb, 64)
        ints += [tiles, tiles * nb + 63, wps]
        zero = Z_NONE
        if not p["yh32"] and not p["band_rows"]:
            zero = Z_F64
        elif p["yh32"] and p["yh_lo"] == 0 and nb < NQ:
            zero = Z_F32
        g.update(fp_q_lo=b["q_lo"], fp_n_main=b["n_main"], fp_n_extra=b["n_extra"], fp_extra_q0=b["extra_q0"], fp_extra_q1=b["extra_q1"],
                 fp_solve0=b["solve0"], fp_nb=nb, fp_tile=best_t, fp_tiles=tiles, fp_wps=wps, fast_km=km, wpc=wpc, zero=zero)
        gx("fast_grid", wps * So)
    elif bins == B_GSS_LANE:
        gx("gss_grid", So * cdiv(NQ, 64))
    elif bins == B_GSS:
        ints.append(So * NQ)
        gx("gss_grid", cdiv(So * NQ, 256 // p["mp"]))
    if p["rec"] == 1 or p["postfilter"]:
        ints.append(So * NQ)
        gx("lane_blocks", cdiv(So * NQ, 64))
    if p["rec"] == 2:
        gx("rec_blocks", So)
    if p["expand"]:
        gx("expand_blocks", cdiv(So * rows * F * N, 256))

    ints.append(Si)
    ist = p["istft"]
    if ist == I_F32:
        slots = max(1, cus * 8 * 2 // Si)
        cps = min(slots, F)
        fpc = cdiv(F, cps)
        cps = cdiv(F, fpc)
        ints += [fpc, cps]
        g.update(per_run=fpc, runs_per_stream=cps)
        gx("istft_grid", cdiv(cps * Si, 8))
    elif ist == I_W64:
        pairs = (F + 1) // 2
        slots = max(1, cus * 4 * 2 // Si)
        rps = min(slots, pairs)
        ppr = cdiv(pairs, rps)
        rps = cdiv(pairs, ppr)
        ints += [ppr, rps]
        g.update(per_run=ppr, runs_per_stream=rps)
        gx("istft_grid", cdiv(rps * Si, 4))
    elif ist == I_SMALL:
        kG = 1024 // N
        L = max(4 * kG, cdiv(cdiv(Si * F, cus * 8), kG) * kG)
        ints.append(L)
        g["per_run"] = L
        gx("istft_grid", cdiv(Si * cdiv(F, L), 8))
    elif ist == I_SPLIT:
        L = max(8, cdiv(Si * F, cus * 8))
        ints.append(L)
        g["per_run"] = L
        gx("istft_grid", cdiv(Si * cdiv(F, L), 8))
    elif ist == I_GENERIC:
        g["per_run"] = 1
        gx("istft_grid", max(1, min(Si * F, cus * 8)))
        gx("ola_grid", cdiv(Si * F * hop, 256))

    tail = p["tail"]
    if tail in (T_SMOOTH4, T_SMOOTH):
        total = F * hop * So
        gx("smooth4_grid", (total // 4 + 255) // 256)
        gx("smooth_grid", cdiv(total, 256))
        gx("state_grid", (64 * So + 255) // 256)
        ints.append(64 * So)
    elif tail != T_NONE:
        fs, nbr = s["gsc_filter_size"], max(1, M - 1)
        kp = p["t1"] if tail in (T_NLMS, T_NLMS_PAR) else p["t2"]
        g["lds_serial"] = 4 * (nbr * ((fs + 64 * kp + 8) | 1) + nbr * ((64 * kp + 8) | 1) + 2 * fs + 16 + nbr * 64 + 64 + 16 + 64)
        g["lds_par"] = 4 * (nbr * ((fs + 64 * kp + 8) | 1) + 2 * fs + 64 * kp + 16 + nbr * 64 + 64 + 64 + 64)
        gx("nlms_grid", S)
    fits = all(0 <= v <= INT_MAX for v in ints) and all(1 <= v <= GX_MAX for v in gxs) and all(1 <= v <= GY_MAX for v in gys)
    return fits, g
