"""Lucas-Kanade restated in numpy, for the tests only (the product never imports it).

transflow's `calc_optical_flow_lukas_kanade` (flow/methods/lukas_kanade.py) makes one OpenCV call,
`cv2.calcOpticalFlowPyrLK(prev, next, p0, p1, winSize=(w, w), maxLevel=L)` with the defaults in force (criteria
COUNT|EPS, 30, 0.01; flags 0; minEigThreshold 1e-4), which writes nextPts in place into p1.  `calc_pyr_lk` restates
OpenCV 4.x's modules/video/src/lkpyramid.cpp statement by statement, vectorised over points; `calc_pyr_lk_scalar` is a
plain per-point transcription of the same statements, kept to cross-check the vectorised form.  `lukas_kanade` is the
reference function around it (grid, in-place p1, kron, crop, dtype).

The image arithmetic is integer and exact.  The float arithmetic is float32, one rounding per operation, in the
source's order; the only choice a real build makes is the order of the float additions of A and b, pinned in one
place: SUM_ORDER.

Points written from memory of the source rather than read from it (to be confirmed against a real OpenCV by
tools/pin_lk_with_cv2.py; until a tests/golden/lk_cv2_*.npz exists this module is parity to a restatement only):

[VERIFY] 1. buildOpticalFlowPyramid(withDerivatives=false): level 0 is the frame copied into a buffer padded by
            winSize with BORDER_REFLECT_101; level l is pyrDown(level l-1) (5x5 [1 4 6 4 1]^2 / 256, (s + 128) >> 8,
            reflect-101 over the level's own size, never reading the pad), padded the same way.
[VERIFY] 2. The level count: after level l, sz = ((w+1)/2, (h+1)/2); if sz.w <= win or sz.h <= win the pyramid stops
            at l, and calcOpticalFlowPyrLK takes that as maxLevel.
[VERIFY] 3. calcSharrDeriv: vertical t0 = (r0+r2)*3 + r1*10, t1 = r2 - r0; horizontal dx = t0[x+1] - t0[x-1],
            dy = (t1[x+1] + t1[x-1])*3 + t1[x]*10; rows and columns reflect-101 (a size of 1 reads itself); then a
            zero border of winSize (copyMakeBorder BORDER_CONSTANT|BORDER_ISOLATED).
[VERIFY] 4. LKTrackerInvoker as summarised in `_track_level`: 14-bit weights by cvRound (half to even), the I patch
            CV_DESCALE(.., 9), the derivative patch CV_DESCALE(.., 14); A = iA * 2^-20; minEig compared as float with
            (float)1e-4; D < FLT_EPSILON; D = 1/D; up to 30 steps; stop on delta.ddot(delta) <= 0.01 * 0.01 (double),
            or for j > 0 on |delta + prevDelta| < 0.01 on both axes after nextPts -= delta * 0.5f.
[VERIFY] 5. acctype and itemtype are float: A and b accumulate in float32.
[VERIFY] 6. SUM_ORDER "simd128" (the x86 build's CV_SIMD128 && !CV_NEON branches):
            A: four lane partials, lane k taking the window column 4c + k of every row (row-major), over the first
            4 * (win // 4) columns; the remaining columns go, row-major, into a scalar accumulator; then
            iA = tail + ((l0 + l2) + (l1 + l3)) (v_reduce_sum).
            b: per row, each 8-column chunk adds float(int32 pair dot products) into two 4-lane partials:
            qb0 = {x: cols 0+4, y: cols 0+4, x: cols 1+5, y: cols 1+5}, qb1 likewise for cols 2+6 and 3+7; the
            remaining columns add float(diff * d) row-major into a scalar accumulator; then
            ib1 = tail1 + ((qb0[0] + qb1[0]) + (qb0[2] + qb1[2])), ib2 likewise with lanes 1 and 3.
            SUM_ORDER "scalar" is the plain loop (no SIMD build): every product added in row-major order.
"""
from __future__ import annotations

import numpy as np

SUM_ORDER = "simd128"            # the one build-dependent choice: "simd128" (x86 CV_SIMD128) or "scalar"

W_BITS = 14
FLT_SCALE = np.float32(1.0 / (1 << 20))
FLT_EPSILON = np.float32(1.1920928955078125e-07)
MIN_EIG = np.float32(1e-4)       # LKTrackerInvoker takes (float)minEigThreshold
MAX_COUNT = 30
EPS2 = 0.01 * 0.01               # criteria.epsilon *= criteria.epsilon (double)

# trace codes of one point at one level
TR_DONE, TR_LOST_PREV, TR_LOST_EIG, TR_LOST_NEXT = 0, 1, 2, 3

# why a point's steps at one level ended (calc_pyr_lk's probe): none were run (TR_LOST_PREV, TR_LOST_EIG), the step
# was at most epsilon, two steps cancelled (the oscillation rule), all MAX_COUNT ran, the window left the frame
STOP_NONE, STOP_EPS, STOP_OSC, STOP_COUNT, STOP_LOST = 0, 1, 2, 3, 4

F32 = np.float32


# ---- images -------------------------------------------------------------------------------------------------------

def border_interpolate(p, n: int):
    """cv::borderInterpolate(p, n, BORDER_REFLECT_101) for an integer array p."""
    p = np.array(p, np.int64, copy=True)
    if n == 1:
        return np.zeros_like(p)
    while True:
        bad = (p < 0) | (p >= n)
        if not bad.any():
            return p
        p = np.where(p < 0, -p, np.where(p >= n, 2 * n - 2 - p, p))


def pad101(img: np.ndarray, pad: int) -> np.ndarray:
    h, w = img.shape
    r = border_interpolate(np.arange(-pad, h + pad), h)
    c = border_interpolate(np.arange(-pad, w + pad), w)
    return img[r][:, c]


def pyr_down(img: np.ndarray) -> np.ndarray:
    """cv2.pyrDown on uint8: 5x5 [1 4 6 4 1]^2, (s + 128) >> 8, reflect-101, size ((w+1)/2, (h+1)/2)."""
    h, w = img.shape
    dh, dw = (h + 1) // 2, (w + 1) // 2
    k = (1, 4, 6, 4, 1)
    src = img.astype(np.int64)
    rows = border_interpolate(2 * np.arange(dh)[:, None] + np.arange(-2, 3)[None, :], h)     # [dh][5]
    cols = border_interpolate(2 * np.arange(dw)[:, None] + np.arange(-2, 3)[None, :], w)
    t = sum(k[j] * src[:, cols[:, j]] for j in range(5))                                     # [h][dw]
    s = sum(k[i] * t[rows[:, i], :] for i in range(5))
    return ((s + 128) >> 8).astype(np.uint8)


def pyr_down_sum(img: np.ndarray) -> np.ndarray:
    """pyr_down's 5x5 sums before the rounding: int64 [(h+1)/2][(w+1)/2]; pyr_down(img) == (sum + 128) >> 8."""
    h, w = img.shape
    dh, dw = (h + 1) // 2, (w + 1) // 2
    k = (1, 4, 6, 4, 1)
    src = img.astype(np.int64)
    rows = border_interpolate(2 * np.arange(dh)[:, None] + np.arange(-2, 3)[None, :], h)
    cols = border_interpolate(2 * np.arange(dw)[:, None] + np.arange(-2, 3)[None, :], w)
    t = sum(k[j] * src[:, cols[:, j]] for j in range(5))
    return sum(k[i] * t[rows[:, i], :] for i in range(5))


def level_count(w: int, h: int, win: int, max_level: int) -> int:
    """The maxLevel buildOpticalFlowPyramid returns."""
    for level in range(max_level + 1):
        w, h = (w + 1) // 2, (h + 1) // 2
        if w <= win or h <= win:
            return level
    return max_level


def pyramid(img: np.ndarray, win: int, max_level: int) -> list:
    """Unpadded levels 0..level_count."""
    n = level_count(img.shape[1], img.shape[0], win, max_level)
    levels = [np.asarray(img, np.uint8)]
    for _ in range(n):
        levels.append(pyr_down(levels[-1]))
    return levels


def scharr(img: np.ndarray):
    """calcSharrDeriv -> (dx, dy) int16 [h][w]."""
    h, w = img.shape
    s = img.astype(np.int64)
    r0, r2 = s[border_interpolate(np.arange(h) - 1, h)], s[border_interpolate(np.arange(h) + 1, h)]
    t0 = (r0 + r2) * 3 + s * 10
    t1 = r2 - r0
    cm, cp = border_interpolate(np.arange(w) - 1, w), border_interpolate(np.arange(w) + 1, w)
    dx = t0[:, cp] - t0[:, cm]
    dy = (t1[:, cp] + t1[:, cm]) * 3 + t1 * 10
    return dx.astype(np.int16), dy.astype(np.int16)


def zero_pad(a: np.ndarray, pad: int) -> np.ndarray:
    return np.pad(a, pad, mode="constant")


# ---- float helpers ------------------------------------------------------------------------------------------------

def cv_round(x):
    """cvRound(float): round half to even (x86 cvtss2si)."""
    return np.rint(np.asarray(x, F32)).astype(np.int64)


def _weights(a, b):
    one, s = F32(1), F32(1 << W_BITS)
    iw00 = cv_round((one - a) * (one - b) * s)
    iw01 = cv_round(a * (one - b) * s)
    iw10 = cv_round((one - a) * b * s)
    iw11 = (1 << W_BITS) - iw00 - iw01 - iw10
    return iw00, iw01, iw10, iw11


def _seq_sum(vals) -> np.ndarray:
    """Float32 sum in the order of the list, from 0."""
    acc = None
    for v in vals:
        v = np.asarray(v, F32)
        acc = v.copy() if acc is None else (acc + v).astype(F32)
    return acc


def _sum_A(p: np.ndarray) -> np.ndarray:
    """p [n][win][win] float32 products (exact) -> the float accumulation iA of SUM_ORDER."""
    n, wh, ww = p.shape
    if SUM_ORDER == "scalar":
        return _seq_sum([p[:, y, x] for y in range(wh) for x in range(ww)]) if wh * ww else np.zeros(n, F32)
    w4 = (ww // 4) * 4
    zero = np.zeros(n, F32)
    tail = _seq_sum([p[:, y, x] for y in range(wh) for x in range(w4, ww)])
    tail = zero if tail is None else tail
    if w4 == 0:
        return tail
    lanes = [_seq_sum([p[:, y, c + k] for y in range(wh) for c in range(0, w4, 4)]) for k in range(4)]
    red = ((lanes[0] + lanes[2]).astype(F32) + (lanes[1] + lanes[3]).astype(F32)).astype(F32)
    return (tail + red).astype(F32)


def _sum_b(diff: np.ndarray, ix: np.ndarray, iy: np.ndarray):
    """diff, ix, iy [n][win][win] int64 -> (ib1, ib2) float32 of SUM_ORDER."""
    n, wh, ww = diff.shape
    px, py = diff * ix, diff * iy                      # exact int products; float() rounds them
    if SUM_ORDER == "scalar":
        return (_seq_sum([px[:, y, x].astype(F32) for y in range(wh) for x in range(ww)]),
                _seq_sum([py[:, y, x].astype(F32) for y in range(wh) for x in range(ww)]))
    w8 = (ww // 8) * 8
    zero = np.zeros(n, F32)
    t1 = _seq_sum([px[:, y, x].astype(F32) for y in range(wh) for x in range(w8, ww)])
    t2 = _seq_sum([py[:, y, x].astype(F32) for y in range(wh) for x in range(w8, ww)])
    t1 = zero if t1 is None else t1
    t2 = zero if t2 is None else t2
    if w8 == 0:
        return t1, t2
    chunks = [(y, c) for y in range(wh) for c in range(0, w8, 8)]
    # lane (k, comp): k = 0..3 the column pair (k, k + 4) of the chunk; comp x or y
    qx = [_seq_sum([(px[:, y, c + k] + px[:, y, c + k + 4]).astype(F32) for (y, c) in chunks]) for k in range(4)]
    qy = [_seq_sum([(py[:, y, c + k] + py[:, y, c + k + 4]).astype(F32) for (y, c) in chunks]) for k in range(4)]
    # qb0 = {qx0, qy0, qx1, qy1}, qb1 = {qx2, qy2, qx3, qy3}; s = qb0 + qb1; reduce pairs (0, 2) and (1, 3)
    xa, xb = (qx[0] + qx[2]).astype(F32), (qx[1] + qx[3]).astype(F32)
    ya, yb = (qy[0] + qy[2]).astype(F32), (qy[1] + qy[3]).astype(F32)
    return (t1 + (xa + xb).astype(F32)).astype(F32), (t2 + (ya + yb).astype(F32)).astype(F32)


def _patch(img_pad: np.ndarray, pad: int, ix, iy, win: int) -> np.ndarray:
    """[n][win+1][win+1] of the padded image at rows iy.., cols ix.. (unpadded coordinates)."""
    r = iy[:, None] + pad + np.arange(win + 1)[None, :]
    c = ix[:, None] + pad + np.arange(win + 1)[None, :]
    return img_pad[r[:, :, None], c[:, None, :]].astype(np.int64)


def _bilinear(patch: np.ndarray, w, shift: int, win: int) -> np.ndarray:
    iw00, iw01, iw10, iw11 = (x[:, None, None] for x in w)
    s = (patch[:, :win, :win] * iw00 + patch[:, :win, 1:] * iw01 + patch[:, 1:, :win] * iw10 + patch[:, 1:, 1:] * iw11)
    return (s + (1 << (shift - 1))) >> shift


# ---- the tracker ----------------------------------------------------------------------------------------------------

def _probe_b(probe, diff, gx, gy):
    """The largest |diff * d| and the largest |pair sum| that SUM_ORDER "simd128" converts to float, into probe."""
    ww = diff.shape[2]
    w8 = (ww // 8) * 8
    for p in (diff * gx, diff * gy):
        probe["max_product"] = max(probe["max_product"], int(np.abs(p).max(initial=0)))
        q = p[:, :, :w8].reshape(p.shape[0], p.shape[1], w8 // 8, 2, 4)
        probe["max_pair_sum"] = max(probe["max_pair_sum"], int(np.abs(q[:, :, :, 0] + q[:, :, :, 1]).max(initial=0)))


def _track_level(level, max_level, I, J, dx, dy, win, prev_pts, next_pts, trace, chunk=2048, probe=None):
    """One parallel_for_ of LKTrackerInvoker over every point (in place on next_pts)."""
    h, w = I.shape
    pad = win
    Ip, Jp = pad101(I, pad), pad101(J, pad)
    Dxp, Dyp = zero_pad(dx, pad), zero_pad(dy, pad)
    half = F32((win - 1) * F32(0.5))
    scale = F32(1.0 / (1 << level))
    for s0 in range(0, len(prev_pts), chunk):
        sl = slice(s0, s0 + chunk)
        prev = (prev_pts[sl] * scale).astype(F32)
        if level == max_level:
            nxt = prev.copy()
        else:
            nxt = (next_pts[sl] * F32(2)).astype(F32)
        next_pts[sl] = nxt
        n = len(prev)
        iters = np.zeros(n, np.int64)
        code = np.full(n, TR_DONE, np.int64)
        prev = (prev - half).astype(F32)
        fl = np.floor(prev.astype(np.float64))
        ok = (fl[:, 0] >= -win) & (fl[:, 0] < w) & (fl[:, 1] >= -win) & (fl[:, 1] < h)
        code[~ok] = TR_LOST_PREV
        idx = np.nonzero(ok)[0]
        if len(idx):
            ipx, ipy = fl[idx, 0].astype(np.int64), fl[idx, 1].astype(np.int64)
            a = (prev[idx, 0] - ipx.astype(F32)).astype(F32)
            b = (prev[idx, 1] - ipy.astype(F32)).astype(F32)
            wts = _weights(a, b)
            ival = _bilinear(_patch(Ip, pad, ipx, ipy, win), wts, W_BITS - 5, win)
            gx = _bilinear(_patch(Dxp, pad, ipx, ipy, win), wts, W_BITS, win)
            gy = _bilinear(_patch(Dyp, pad, ipx, ipy, win), wts, W_BITS, win)
            fx, fy = gx.astype(F32), gy.astype(F32)
            A11 = (_sum_A((fx * fx).astype(F32)) * FLT_SCALE).astype(F32)
            A12 = (_sum_A((fx * fy).astype(F32)) * FLT_SCALE).astype(F32)
            A22 = (_sum_A((fy * fy).astype(F32)) * FLT_SCALE).astype(F32)
            D = (A11 * A22 - A12 * A12).astype(F32)
            d = (A11 - A22).astype(F32)
            root = np.sqrt(((d * d).astype(F32) + ((F32(4) * A12).astype(F32) * A12).astype(F32)).astype(F32))
            min_eig = (((A22 + A11).astype(F32) - root).astype(F32) / F32(2 * win * win)).astype(F32)
            good = ~((min_eig < MIN_EIG) | (D < FLT_EPSILON))
            code[idx[~good]] = TR_LOST_EIG
            if probe is not None:
                probe["min_eig"][s0 + idx, level] = min_eig
                probe["det"][s0 + idx, level] = D
            sel = np.nonzero(good)[0]
            idx = idx[sel]
            ival, gx, gy = ival[sel], gx[sel], gy[sel]
            A11, A12, A22 = A11[sel], A12[sel], A22[sel]
            D = (F32(1) / D[sel]).astype(F32)
            pt = (nxt[idx] - half).astype(F32)
            prev_delta = np.zeros((len(idx), 2), F32)
            live = np.ones(len(idx), bool)
            for j in range(MAX_COUNT):
                li = np.nonzero(live)[0]
                if not len(li):
                    break
                fn = np.floor(pt[li].astype(np.float64))
                inb = (fn[:, 0] >= -win) & (fn[:, 0] < w) & (fn[:, 1] >= -win) & (fn[:, 1] < h)
                code[idx[li[~inb]]] = TR_LOST_NEXT
                live[li[~inb]] = False
                if probe is not None:
                    probe["stop"][s0 + idx[li[~inb]], level] = STOP_LOST
                li = li[inb]
                if not len(li):
                    break
                fn = fn[inb]
                inx, iny = fn[:, 0].astype(np.int64), fn[:, 1].astype(np.int64)
                a = (pt[li, 0] - inx.astype(F32)).astype(F32)
                b = (pt[li, 1] - iny.astype(F32)).astype(F32)
                jval = _bilinear(_patch(Jp, pad, inx, iny, win), _weights(a, b), W_BITS - 5, win)
                diff = jval - ival[li]
                ib1, ib2 = _sum_b(diff, gx[li], gy[li])
                if probe is not None:
                    _probe_b(probe, diff, gx[li], gy[li])
                b1, b2 = (ib1 * FLT_SCALE).astype(F32), (ib2 * FLT_SCALE).astype(F32)
                ddx = (((A12[li] * b2).astype(F32) - (A22[li] * b1).astype(F32)).astype(F32) * D[li]).astype(F32)
                ddy = (((A12[li] * b1).astype(F32) - (A11[li] * b2).astype(F32)).astype(F32) * D[li]).astype(F32)
                pt[li, 0] = (pt[li, 0] + ddx).astype(F32)
                pt[li, 1] = (pt[li, 1] + ddy).astype(F32)
                gi = s0 + idx[li]
                next_pts[gi] = (pt[li] + half).astype(F32)
                iters[idx[li]] = j + 1
                dd = ddx.astype(np.float64) * ddx.astype(np.float64) + ddy.astype(np.float64) * ddy.astype(np.float64)
                stop = dd <= EPS2
                if j > 0:
                    osc = ((np.abs((ddx + prev_delta[li, 0]).astype(F32)).astype(np.float64) < 0.01)
                           & (np.abs((ddy + prev_delta[li, 1]).astype(F32)).astype(np.float64) < 0.01) & ~stop)
                    oi = np.nonzero(osc)[0]
                    if len(oi):
                        g = gi[oi]
                        next_pts[g, 0] = (next_pts[g, 0] - (ddx[oi] * F32(0.5)).astype(F32)).astype(F32)
                        next_pts[g, 1] = (next_pts[g, 1] - (ddy[oi] * F32(0.5)).astype(F32)).astype(F32)
                    stop = stop | osc
                if probe is not None:
                    probe["stop"][gi, level] = np.where(dd <= EPS2, STOP_EPS, np.where(stop, STOP_OSC, STOP_COUNT))
                live[li[stop]] = False
                prev_delta[li, 0] = ddx
                prev_delta[li, 1] = ddy
        if trace is not None:
            trace[sl, level, 0:2] = next_pts[sl]
            trace[sl, level, 2] = iters
            trace[sl, level, 3] = code


def calc_pyr_lk(prev: np.ndarray, nxt: np.ndarray, pts: np.ndarray, win: int, max_level: int, with_trace=False,
                probe=None):
    """cv2.calcOpticalFlowPyrLK(prev, next, pts, None, winSize=(win, win), maxLevel=max_level)[0] with the default
    criteria and flags: nextPts [n][2] float32 (whatever the status).  with_trace: also [n][levels][4] float64
    {nextPts.x, nextPts.y, steps run, code} after each level (index = level).  probe: a dict that receives "stop"
    [n][levels] (a STOP_* per point and level), "min_eig" and "det" [n][levels] float32 (NaN where TR_LOST_PREV), and
    "max_product" and "max_pair_sum", the largest integers |diff * d| and |diff_k * d_k + diff_k+4 * d_k+4| of b."""
    assert win > 2 and max_level >= 0
    pts = np.asarray(pts, F32).reshape(-1, 2)
    L = level_count(prev.shape[1], prev.shape[0], win, max_level)
    pp, pn = pyramid(prev, win, L), pyramid(nxt, win, L)
    next_pts = pts.copy()
    trace = np.zeros((len(pts), L + 1, 4)) if with_trace else None
    if probe is not None:
        probe.update(stop=np.full((len(pts), L + 1), STOP_NONE, np.int64), max_product=0, max_pair_sum=0,
                     min_eig=np.full((len(pts), L + 1), np.nan, F32), det=np.full((len(pts), L + 1), np.nan, F32))
    for level in range(L, -1, -1):
        dx, dy = scharr(pp[level])
        _track_level(level, L, pp[level], pn[level], dx, dy, win, pts, next_pts, trace, probe=probe)
    return (next_pts, trace) if with_trace else next_pts


# ---- the same, one point at a time ------------------------------------------------------------------------------------

def calc_pyr_lk_scalar(prev: np.ndarray, nxt: np.ndarray, pts: np.ndarray, win: int, max_level: int) -> np.ndarray:
    """A plain transcription of LKTrackerInvoker::operator() for each point, loop by loop (the SIMD loops lane by
    lane).  Slow: for cross-checking calc_pyr_lk on a few hundred points."""
    pts = np.asarray(pts, F32).reshape(-1, 2)
    L = level_count(prev.shape[1], prev.shape[0], win, max_level)
    pp, pn = pyramid(prev, win, L), pyramid(nxt, win, L)
    out = pts.copy()
    half = F32((win - 1) * F32(0.5))
    simd = SUM_ORDER == "simd128"
    for level in range(L, -1, -1):
        I, J = pp[level], pn[level]
        h, w = I.shape
        Ip, Jp = pad101(I, win).astype(np.int64), pad101(J, win).astype(np.int64)
        dxs, dys = scharr(I)
        Dx, Dy = zero_pad(dxs, win).astype(np.int64), zero_pad(dys, win).astype(np.int64)
        scale = F32(1.0 / (1 << level))
        for i in range(len(pts)):
            px, py = F32(pts[i, 0] * scale), F32(pts[i, 1] * scale)
            if level == L:
                nx, ny = px, py
            else:
                nx, ny = F32(out[i, 0] * F32(2)), F32(out[i, 1] * F32(2))
            out[i] = (nx, ny)
            px, py = F32(px - half), F32(py - half)
            ix, iy = int(np.floor(px)), int(np.floor(py))
            if ix < -win or ix >= w or iy < -win or iy >= h:
                continue
            a, b = F32(px - F32(ix)), F32(py - F32(iy))
            w00, w01, w10, w11 = (int(v) for v in _weights(a, b))

            def interp(img, r, c, shift, ww=(w00, w01, w10, w11)):
                r, c = r + win, c + win
                s = img[r, c] * ww[0] + img[r, c + 1] * ww[1] + img[r + 1, c] * ww[2] + img[r + 1, c + 1] * ww[3]
                return (int(s) + (1 << (shift - 1))) >> shift
            Iw = [[0] * win for _ in range(win)]
            Gx = [[0] * win for _ in range(win)]
            Gy = [[0] * win for _ in range(win)]
            iA = [F32(0)] * 3
            qA = [[F32(0)] * 4 for _ in range(3)]
            w4 = (win // 4) * 4 if simd else 0
            for y in range(win):
                for x in range(win):
                    Iw[y][x] = interp(Ip, iy + y, ix + x, W_BITS - 5)
                    Gx[y][x] = interp(Dx, iy + y, ix + x, W_BITS)
                    Gy[y][x] = interp(Dy, iy + y, ix + x, W_BITS)
                    fx, fy = F32(Gx[y][x]), F32(Gy[y][x])
                    prods = (F32(fx * fx), F32(fx * fy), F32(fy * fy))
                    for k in range(3):
                        if x < w4:
                            qA[k][x % 4] = F32(qA[k][x % 4] + prods[k])
                        else:
                            iA[k] = F32(iA[k] + prods[k])
            if simd and w4:
                for k in range(3):
                    q = qA[k]
                    iA[k] = F32(iA[k] + F32(F32(q[0] + q[2]) + F32(q[1] + q[3])))
            A11, A12, A22 = (F32(v * FLT_SCALE) for v in iA)
            D = F32(F32(A11 * A22) - F32(A12 * A12))
            min_eig = F32(F32(F32(A22 + A11) - np.sqrt(F32(F32(F32(A11 - A22) * F32(A11 - A22))
                                                         + F32(F32(F32(4) * A12) * A12))))
                          / F32(2 * win * win))
            if min_eig < MIN_EIG or D < FLT_EPSILON:
                continue
            D = F32(F32(1) / D)
            nx, ny = F32(nx - half), F32(ny - half)
            pdx = pdy = F32(0)
            for j in range(MAX_COUNT):
                jx, jy = int(np.floor(nx)), int(np.floor(ny))
                if jx < -win or jx >= w or jy < -win or jy >= h:
                    break
                a, b = F32(nx - F32(jx)), F32(ny - F32(jy))
                v00, v01, v10, v11 = (int(v) for v in _weights(a, b))
                ib1 = ib2 = F32(0)
                qb = [F32(0)] * 8          # qb0 lanes 0..3, qb1 lanes 0..3
                w8 = (win // 8) * 8 if simd else 0
                for y in range(win):
                    for x in range(win):
                        r, c = jy + y + win, jx + x + win
                        jv = (int(Jp[r, c] * v00 + Jp[r, c + 1] * v01 + Jp[r + 1, c] * v10 + Jp[r + 1, c + 1] * v11)
                              + (1 << 8)) >> 9
                        diff = jv - Iw[y][x]
                        if x < w8:
                            continue
                        ib1 = F32(ib1 + F32(diff * Gx[y][x]))
                        ib2 = F32(ib2 + F32(diff * Gy[y][x]))
                    for c in range(0, w8, 8):
                        dif = []
                        for k in range(8):
                            r, cc = jy + y + win, jx + c + k + win
                            jv = (int(Jp[r, cc] * v00 + Jp[r, cc + 1] * v01 + Jp[r + 1, cc] * v10
                                      + Jp[r + 1, cc + 1] * v11) + (1 << 8)) >> 9
                            dif.append(jv - Iw[y][c + k])
                        for k in range(4):
                            lane = (k // 2) * 4 + (k % 2) * 2     # qb0: k 0, 1 -> lanes 0, 2; qb1: k 2, 3 -> 0, 2
                            sx = dif[k] * Gx[y][c + k] + dif[k + 4] * Gx[y][c + k + 4]
                            sy = dif[k] * Gy[y][c + k] + dif[k + 4] * Gy[y][c + k + 4]
                            qb[lane] = F32(qb[lane] + F32(sx))
                            qb[lane + 1] = F32(qb[lane + 1] + F32(sy))
                if simd and w8:
                    s = [F32(qb[k] + qb[4 + k]) for k in range(4)]
                    ib1 = F32(ib1 + F32(s[0] + s[2]))
                    ib2 = F32(ib2 + F32(s[1] + s[3]))
                b1, b2 = F32(ib1 * FLT_SCALE), F32(ib2 * FLT_SCALE)
                ddx = F32(F32(F32(A12 * b2) - F32(A22 * b1)) * D)
                ddy = F32(F32(F32(A12 * b1) - F32(A11 * b2)) * D)
                nx, ny = F32(nx + ddx), F32(ny + ddy)
                out[i] = (F32(nx + half), F32(ny + half))
                if float(ddx) * float(ddx) + float(ddy) * float(ddy) <= EPS2:
                    break
                if j > 0 and abs(float(F32(ddx + pdx))) < 0.01 and abs(float(F32(ddy + pdy))) < 0.01:
                    out[i] = (F32(out[i, 0] - F32(ddx * F32(0.5))), F32(out[i, 1] - F32(ddy * F32(0.5))))
                    break
                pdx, pdy = ddx, ddy
    return out


# ---- the reference function ------------------------------------------------------------------------------------------

def grid_points(h: int, w: int, step: int) -> np.ndarray:
    p0 = np.stack(np.meshgrid(np.arange(0, w, step), np.arange(0, h, step), indexing="xy"), axis=-1).astype(F32)
    return p0.reshape(-1, 2)


def expand(flow_pts: np.ndarray, h: int, w: int, step: int) -> np.ndarray:
    """[q][p][2] point flows -> the reference's [h][w][2] float32 (kron by step, crop)."""
    if step == 1:
        return flow_pts
    return np.kron(flow_pts, np.ones((step, step, 1)))[0:h, 0:w, :].astype(flow_pts.dtype)


def lukas_kanade(prev: np.ndarray, nxt: np.ndarray, win_size: int, max_level: int, step: int) -> np.ndarray:
    """calc_optical_flow_lukas_kanade(prev, next, win_size, max_level, step)."""
    h, w = prev.shape
    p0 = grid_points(h, w, step)
    q, p = len(range(0, h, step)), len(range(0, w, step))
    p1 = calc_pyr_lk(prev, nxt, p0, win_size, max_level)
    return expand((p1 - p0).reshape(q, p, 2), h, w, step)


def lukas_kanade_at(prev, nxt, win_size, max_level, step, point_index):
    """The reference function's flow at the grid points point_index only (points are independent): [k][2]."""
    h, w = prev.shape
    p0 = grid_points(h, w, step)[np.asarray(point_index)]
    return calc_pyr_lk(prev, nxt, p0, win_size, max_level) - p0
