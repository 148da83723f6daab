"""Plain reference of the read stage's sizing pass (k_phase_bounds) and of the reduction of its bounds (k_bounds_reduce).

Written from the RULES of phase_body.hpp: uz_phase_bounds_w -- which record ranges a DNM's own fetch and its het-site fetches cover -- with
np.searchsorted over the contig's start column as the only search.  Nothing of the index (coarse / mid / mid8 levels, the staged entries of the
kernel) appears in `sizing` and `reduce_bounds`; `branch_stats` at the end re-derives which branch of the kernel a DNM reaches, for the
coverage statements of the tests only -- no expected value comes from it."""
import numpy as np

VT_POINT = 0
DF_FETCH_FALLBACK = 1
T_CAP = 0x7FFFFFF0
I32_MAX = 0x7FFFFFFF


def _clamp(v):
    """uz_clamp_i32: starts are int32, a value beyond either end compares like the end"""
    return max(-I32_MAX, min(I32_MAX, int(v)))


def sizing(start, contig_off, max_span, pos, rcontig, dstart, dend, vartype, dflags, cutoff, cand_off, het_off, het_idx, no_extended=False):
    """-> dict(bounds [n, 5], pre_win [n, 4], pre_ha [n_het], pre_hl [n_het])"""
    start = np.asarray(start, np.int64)
    pos = np.asarray(pos, np.int64)
    n = len(rcontig)
    n_het = int(het_off[n])
    bounds, pre_win = np.zeros((n, 5), np.int64), np.zeros((n, 4), np.int64)
    pre_ha, pre_hl = np.zeros(n_het, np.int64), np.zeros(n_het, np.int64)
    icut = int(cutoff)  # uz_cutoff is a double, the windows take its integer part
    for d in range(n):
        nc, nh = int(cand_off[d + 1] - cand_off[d]), int(het_off[d + 1] - het_off[d])
        bounds[d, 2], bounds[d, 3] = nh, nc
        if nc == 0:
            continue
        tid = int(rcontig[d])
        ok = 0 <= tid < len(contig_off) - 1
        clo, chi = (int(contig_off[tid]), int(contig_off[tid + 1])) if ok else (0, 0)
        span = int(max_span[tid]) if ok else 0
        col = start[clo:chi]

        def lb(v):
            return int(np.searchsorted(col, _clamp(v), "left")) + clo

        if int(vartype[d]) == VT_POINT:
            flo = int(dstart[d]) if (int(dflags[d]) & DF_FETCH_FALLBACK) else int(dstart[d]) - 1
            if ok:
                ra = lb(flo - span)
                rb = max(ra, lb(int(dstart[d]) + 1))
                bounds[d, 0] = rb - ra
                pre_win[d] = (ra, rb, 0, 0)
        elif ok:  # +-cutoff around both breakpoints, the lows clipped at 0
            lo1, lo2 = max(0, int(dstart[d]) - icut), max(0, int(dend[d]) - icut)
            fa, fa2 = lb(lo1 - span), lb(lo2 - span)
            fb, fb2 = max(fa, lb(int(dstart[d]) + icut)), max(fa2, lb(int(dend[d]) + icut))
            bounds[d, 0] = (fb - fa) + (fb2 - fa2)
            pre_win[d] = (fa, fb, fa2, fb2)
        if no_extended:
            continue
        h0 = int(het_off[d])
        hp = pos[np.asarray(het_idx[h0:h0 + nh], np.int64)]
        total = 0
        for h in range(nh):
            if ok:
                a = lb(int(hp[h]) - span)
                ln = max(0, lb(int(hp[h]) + 1) - a)
                pre_ha[h0 + h], pre_hl[h0 + h] = a, ln
                total += ln
            left = h  # first het site (sorted) a record ending at hp could still reach back to
            while left > 0 and int(hp[left - 1]) >= int(hp[h]) - span - 1:
                left -= 1
            bounds[d, 4] = max(bounds[d, 4], h - left + 1)
        bounds[d, 1] = min(total, T_CAP)
    return dict(bounds=bounds.astype(np.int32), pre_win=pre_win.astype(np.int32), pre_ha=pre_ha.astype(np.int32), pre_hl=pre_hl.astype(np.int32))


def reduce_bounds(bounds):
    """k_bounds_reduce, from its comment block: the maxima, M = b1 + 4 b0 (b4 + 1), the sum of min(M, 4096) + b3, the DNMs with candidates and the
    histogram of their arena estimates in units of 256 bytes"""
    b = np.asarray(bounds, np.int64).reshape(-1, 5)
    b0, b1, b2, b3, b4 = (b[:, k] for k in range(5))
    M = b1 + 4 * b0 * (b4 + 1)
    act = b3 > 0
    est = np.minimum(((37 * b1[act]) // 4 + 10 * b0[act] + 3328 + 255) >> 8, 255)
    z = lambda x: int(x.max()) if x.size else 0  # noqa: E731
    return dict(mA=z(b0), mT=z(b1), mH=z(b2), mC=z(b3), active=int(act.sum()), mM=z(M), sumP=int((np.minimum(M, 4096) + b3).sum()),
                hist=np.bincount(est, minlength=256).astype(np.int64))


# ---------------------------------------------------------------- which branch of k_phase_bounds a DNM reaches (coverage statements only)
STAGE = 64  # UZ_BW_STAGE


def branch_stats(start, contig_off, max_span, pos, rcontig, dstart, vartype, dflags, cand_off, het_off, het_idx, no_extended=False):
    """Per DNM with candidates on a contig of more than 128 records (the others take uz_lower_bounds_c chain by chain): is the coarse level used,
    how many mid entries are staged, do they reach the contig's end (`whole`), how many of its chains lie beyond them (`far`).  From the kernel's
    own rule -- the stage starts at the last 64-record cell boundary at or below the lower bound of the DNM's lowest value, clipped to the
    contig's mid entries -- with searchsorted for the lower bounds."""
    start = np.asarray(start, np.int64)
    pos = np.asarray(pos, np.int64)
    out = []
    for d in range(len(rcontig)):
        nc, nh = int(cand_off[d + 1] - cand_off[d]), int(het_off[d + 1] - het_off[d])
        tid = int(rcontig[d])
        ok = 0 <= tid < len(contig_off) - 1
        clo, chi = (int(contig_off[tid]), int(contig_off[tid + 1])) if ok else (0, 0)
        if nc == 0 or chi - clo <= 128:
            out.append(dict(shared=False, mid=ok and chi - clo > 128, coarse=False, staged=None, whole=None, far=0, records=chi - clo))
            continue
        span = int(max_span[tid])
        col = start[clo:chi]
        lb = lambda v: int(np.searchsorted(col, _clamp(v), "left")) + clo  # noqa: E731
        point = int(vartype[d]) == VT_POINT
        vals = []
        if point:
            p = int(dstart[d])
            vals += [(p if int(dflags[d]) & DF_FETCH_FALLBACK else p - 1) - span, p + 1]
        if not no_extended:
            for h in range(nh):
                hp = int(pos[int(het_idx[int(het_off[d]) + h])])
                vals += [hp - span, hp + 1]
        kl_m, kh_m = (clo + 63) >> 6, chi >> 6
        if not vals:
            out.append(dict(shared=True, mid=True, coarse=chi - clo > 8192, staged=None, whole=None, far=0, records=chi - clo))
            continue
        r0 = lb(min(vals))
        # entries of the mid index below the lowest value: mid[k] = start[64 k] < vmin  <=>  64 k < r0
        below = max(kl_m, min(kh_m, (r0 + 63) >> 6))
        s0 = max(kl_m, below - 1) if below > kl_m else kl_m
        s_end = max(s0, min(s0 + STAGE, kh_m))
        whole = s_end == kh_m
        # a chain is far when every staged entry lies below its value (and the stage stops short of the contig's end)
        far = 0 if whole else sum(1 for v in vals if s_end == s0 or int(start[(s_end - 1) << 6]) < _clamp(v))
        out.append(dict(shared=True, mid=True, coarse=chi - clo > 8192, staged=s_end - s0, whole=whole, far=far, records=chi - clo))
    return out
