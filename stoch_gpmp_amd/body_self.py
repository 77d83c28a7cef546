"""Host-side twin (numpy) of the body's self-collision term, SGPMP_COST_BODY_SELF (include/sgpmp.h has the definition;
csrc/body_self_device.h evaluates it on the device), operation for operation: for tests, examples and host-side checks.  No
reference counterpart.  `body` is a robots.body.BodySpheres (or anything with `links`, `centers`, `radii`); `rows` are the rows of
sgpmp_set_body_pairs (BodySpheres.pair_rows): one integer per sphere, bit j of rows[i] set = pair (i, j) counted, j > i."""
import numpy as np

from .body_sdf import body_points, link_frames


def pair_rows(links, min_link_gap=2, ignore=()):
    """Link indices [M] (non-decreasing) -> the rows: pairs whose link indices differ by at least `min_link_gap`, without the
    link pairs listed in `ignore`.  ValueError when nothing is counted."""
    if min_link_gap < 1:
        raise ValueError("pair_rows: min_link_gap must be >= 1 (a pair on one link is a constant)")
    links = [int(v) for v in links]
    skip = {(min(int(a), int(b)), max(int(a), int(b))) for a, b in ignore}
    rows = [0] * len(links)
    for i in range(len(links)):
        for j in range(i + 1, len(links)):
            lo, hi = min(links[i], links[j]), max(links[i], links[j])
            if hi - lo >= min_link_gap and (lo, hi) not in skip:
                rows[i] |= 1 << j
    if not any(rows):
        raise ValueError("pair_rows: no pair is counted")
    return rows


def pair_list(rows):
    """rows -> [(i, j)] in summation order: i ascending, then j ascending; only bits j > i."""
    n = len(rows)
    return [(i, j) for i in range(n) for j in range(i + 1, n) if int(rows[i]) >> j & 1]


def clearance(frames, body, rows):
    """Link frames [..., L, 4, 4] -> s [..., N] = |p_i - p_j| - r_i - r_j over the counted pairs, in summation order, in the
    dtype of `frames`; a non-finite coordinate gives NaN."""
    return field(0., frames, body, rows)[2]


def field(margin, frames, body, rows):
    """-> (f [...], h [..., N], s [..., N], g [..., N, 3]): h = (margin + r_i + r_j) - D where positive, else 0, f = sum h in
    summation order, s the clearance and g = dh/dp_j = (p_i - p_j) / D (dh/dp_i is its negative), exactly zero where the hinge
    is inactive and where D = 0.  In the dtype of `frames`."""
    frames = np.asarray(frames)
    real = frames.dtype.type
    pts = body_points(frames, body)
    r = np.asarray(body.radii, dtype=frames.dtype)
    pairs = pair_list(rows)
    i, j = np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs])
    with np.errstate(invalid="ignore", divide="ignore"):
        d = pts[..., i, :] - pts[..., j, :]
        D = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
        bad = ~np.isfinite(D)
        D = np.where(bad, real(np.nan), D)
        e = ((real(margin) + r[i]) + r[j]) - D
        on = e > 0
        h = np.where(on, e, real(0.))
        h = np.where(bad, real(np.nan), h)
        g = np.where((on & (D > 0))[..., None], d / np.where(D > 0, D, real(1.))[..., None], real(0.))
        g = np.where(bad[..., None], real(np.nan), g)
        f = np.zeros(h.shape[:-1], dtype=frames.dtype)
        for k in range(h.shape[-1]):
            f = f + h[..., k]
        s = (D - r[i]) - r[j]
    return f, h, s, g


def config_field(margin, q, chain, body, rows, dtype=np.float64):
    """q [B, n] -> (f [B], df/dq [B, n], min s [B], its gradient through the first arg-min pair [B, n]): a pair adds
    z_k . ((p_j - o_k) x g) to the revolute joints link_i <= k < link_j (for a joint in front of both links the two forces cancel).
    A non-finite coordinate of a counted sphere makes the value and every gradient entry NaN."""
    frames, z, o = link_frames(q, chain, dtype)
    f, h, s, g = field(margin, frames, body, rows)
    pts = body_points(frames, body)
    pairs = pair_list(rows)
    links = np.asarray(body.links)
    B, n = frames.shape[0], sum(1 for j in chain if j[1] == "revolute")
    rows_b = np.arange(B)
    with np.errstate(invalid="ignore", divide="ignore"):
        best = np.zeros(B, dtype=np.int64)            # first arg-min, strict comparison
        smin = np.full(B, np.inf, dtype=frames.dtype)
        for k in range(len(pairs)):
            better = s[:, k] < smin
            smin = np.where(better, s[:, k], smin)
            best = np.where(better, k, best)
        bi, bj = np.array([p[0] for p in pairs])[best], np.array([p[1] for p in pairs])[best]
        d = pts[rows_b, bi] - pts[rows_b, bj]
        D = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        gq = np.where((D > 0)[:, None], -d / np.where(D > 0, D, 1.)[:, None], 0.)        # ds/dp_j
        grad, gmin = np.zeros((B, n), dtype=frames.dtype), np.zeros((B, n), dtype=frames.dtype)
        col = 0
        for k, (_, kind, _, _) in enumerate(chain):
            if kind != "revolute":
                continue
            for m, (i, j) in enumerate(pairs):
                if links[i] <= k < links[j]:
                    grad[:, col] += np.einsum("bi,bi->b", z[:, k], np.cross(pts[:, j] - o[:, k], g[:, m]))
            between = (links[bi] <= k) & (k < links[bj])
            t = np.einsum("bi,bi->b", z[:, k], np.cross(pts[rows_b, bj] - o[:, k], gq))
            gmin[:, col] = np.where(between, t, 0.)
            col += 1
    nan = np.isnan(s).any(-1)
    f = np.where(nan, np.nan, f)
    grad[nan], gmin[nan] = np.nan, np.nan
    smin = np.where(nan, np.nan, smin)
    return f, grad, smin, gmin
