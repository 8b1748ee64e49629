"""Scans that take the LOAM-style (ROT) extractor (lili_extract_rot.hip) through the branches no synthetic scan reaches: start azimuths in every quadrant
and sweeps on either side of pi (both endOri corrections, the four wrap branches), the `halfPassed` latch at workgroup edges, relTime outside [0, 1], the three
ring tables at every id boundary, row counts around one workgroup and beyond the one-trip histogram sum, ring lengths at the LDS working set and at the
thresholds in ring length, greedy picks at their caps, marks spilled over segment borders (wait, redo, chained redo), the near-range branch, the voxel
ordering at its packed-key limits, sort ties and the slerp's branches.

Shared by tests/test_rot_cases_cpu.py (the conditions on the inputs, on the oracle alone), tests/test_rot_branches_gpu.py (the device against the oracle) and
tests/golden/make_ref_golden.py (the oracle against the reference's own Preprocessing.cpp).  Referee: oracle.extract_rot.  azimuth_model and
greedy_segment are numpy restatements of oracle/lo_extract.cpp:136-171 and of ONE segment's greedy run (:208-245) whose only purpose is to say in which
branch a case is and by what margin.

A case: dict(name, family, raw (n x 4 float32, firing order), n_scans, ds_rate, ds_v, near_range, q_imu, q_lb, claim, ref).  ref: the case takes part in
the comparison with the literal reference build (parameters the node can express, no sort ties).

Geometry of a constructed ring: the point at azimuth `ori` (ori = -atan2(y, x), increasing with time) and horizontal range rho on the ring of elevation e is
(rho cos ori, -rho sin ori, rho tan e).  A `spike` moves one point radially by h: its 11-tap curvature is (10 h)^2, that of its ten neighbours h^2, the squared
gap to its neighbours h^2 + step^2 — h = 0.17 .. 0.205 gives curvature > 2.8 with gaps < 0.045 (marks pass), h >= 0.25 gaps > 0.06 (marks stop)."""
import functools

import numpy as np

from lili_om_amd import synth

INT_MAX = 0x7fffffff
IDENTITY = (1.0, 0.0, 0.0, 0.0)
Q_LB = (0.7071, 0.0, 0.0, 0.7071)                          # R/config/config_fr_iosb.yaml:38-41 (not unit norm)
_A = 0.03
Q_SMALL = (np.cos(_A / 2), np.sin(_A / 2) * 0.3, -np.sin(_A / 2) * 0.5, np.sin(_A / 2) * 0.81)
TABLE16 = -15.0 + 2.0 * np.arange(16)                      # id = int((angle + 15) / 2 + 0.5)
ELEV64 = synth.hdl64_elevations_deg()
ELEV64[0] = 1.9                                            # (ring 0 of the synthetic sensor sits ON the table's upper limit of 2 deg: here inside it, still id 0)
FAMILIES = ("sweep", "latch", "reltime", "tables", "sizes", "picks", "borders", "near", "voxels", "ties", "slerp")
CURV_SHARP, CURV_FLAT, GAP_BREAK = 2.0, 0.1, 0.05
LDS_CAP = 4096                                             # kRingLdsCap
ONE_TRIP_ROWS = 262144                                     # k_rot_scatter: sixteen histogram loads per wave and trip
PI = np.pi


def case(name, family, raw, n_scans=64, ds_rate=1, ds_v=0.6, near_range=3.0, q_imu=IDENTITY, q_lb=IDENTITY, claim=None, ref=True):
    assert family in FAMILIES
    raw = np.ascontiguousarray(raw, np.float32)
    assert raw.ndim == 2 and raw.shape[1] == 4 and raw.shape[0] <= 300_000
    f = raw[np.isfinite(raw).all(axis=1)]
    assert f.shape[0] == 0 or np.abs(f[:, :3]).max() < 1e4
    ref = bool(ref and near_range == 3.0 and ds_v == 0.6)
    return dict(name=name, family=family, raw=raw, n_scans=n_scans, ds_rate=ds_rate, ds_v=ds_v, near_range=near_range, q_imu=tuple(q_imu), q_lb=tuple(q_lb),
                claim=claim or {}, ref=ref)


def oracle_params(oracle, c, atan_mode=2, stable_sort=1, ds_rate=None):
    return oracle.rot_params(n_scans=c["n_scans"], ds_rate=ds_rate or c["ds_rate"], ds_v=c["ds_v"], near_thres=c["near_range"], atan_mode=atan_mode,
                             stable_sort=stable_sort)


def run_oracle(oracle, c, atan_mode=2, stable_sort=1):
    return oracle.extract_rot(c["raw"], c["q_imu"], c["q_lb"], oracle_params(oracle, c, atan_mode, stable_sort))


# ------------------------------------------------------------------------------------------------
# builders
# ------------------------------------------------------------------------------------------------
def ring_rows(ori, rho, elev_deg, refl=10.0):
    ori, rho = np.asarray(ori, np.float64), np.asarray(rho, np.float64)
    e = np.deg2rad(np.asarray(elev_deg, np.float64))
    out = np.empty((ori.shape[0], 4), np.float32)
    out[:, 0] = rho * np.cos(ori)
    out[:, 1] = -rho * np.sin(ori)
    out[:, 2] = rho * np.tan(e)
    out[:, 3] = refl
    return out


def interleave(rings):
    """Rings of different lengths merged the way a spinning sensor fires them: by the fraction of the revolution, then by ring; every ring keeps its order."""
    frac = np.concatenate([(np.arange(r.shape[0]) + 0.5) / max(r.shape[0], 1) for r in rings])
    which = np.concatenate([np.full(r.shape[0], k) for k, r in enumerate(rings)])
    order = np.lexsort((which, frac))
    return np.concatenate(rings)[order]


def room_rho(ori, elev_deg, half=30.0, height=1.8):
    """Horizontal range in a square room of half-size `half` with the floor `height` below the sensor: walls, four corners, eleven pillars 1.5 m in front of
    the walls, a floor line on the low rings."""
    ori = np.asarray(ori, np.float64)
    r = half / np.maximum(np.abs(np.cos(ori)), np.abs(np.sin(ori)))
    r = r - 1.5 * ((ori * 11 / (2 * PI)) % 1.0 < 0.04)
    e = np.deg2rad(np.asarray(elev_deg, np.float64))
    with np.errstate(divide="ignore"):
        g = np.where(e < 0, height / np.tan(-np.minimum(e, -1e-9)), np.inf)
    return np.minimum(r, g)


def segment_bounds(count, j, base=0):
    """sp, ep of segment j of a ring with `count` points whose first point has index `base` (lo_extract.cpp:180-183, 209-210)."""
    rs, re = base + 5, base + count - 6
    return rs + (re - rs) * j // 6, rs + (re - rs) * (j + 1) // 6 - 1


@functools.lru_cache(maxsize=None)
def scene_scan(start=0.8, sweep=2 * PI, n_az=200, elev="hdl64", seed=0, scene="outdoor"):
    """An ordinary scan of the outdoor scene (or of room_rho's room: no ray casting), azimuth-major: row = step * rings + ring, WHATEVER returns (a ray
    without a return is a NaN row), 2 cm range noise.  -> (raw, ori per row, ring per row)."""
    el = {"hdl64": ELEV64, "ids51": ELEV64[:51], "hdl32": synth.hdl32_elevations_deg(), "vlp16": TABLE16}[elev]
    ori = start + sweep * np.arange(n_az) / n_az
    a, e = np.repeat(ori, len(el)), np.tile(np.deg2rad(el), n_az)
    d = np.stack([np.cos(e) * np.cos(a), -np.cos(e) * np.sin(a), np.sin(e)], 1)
    if scene == "room":
        t = room_rho(a, np.tile(el, n_az)) / np.cos(e)
    else:
        t = synth.OutdoorScene().raycast(np.array([0.0, 0.0, 1.8]), d)
    rng = np.random.default_rng(900 + seed)
    t = t + rng.normal(0, 0.02, t.shape)
    raw = np.concatenate([d * t[:, None], rng.integers(1, 255, (t.shape[0], 1)).astype(np.float64)], 1).astype(np.float32)
    raw[~np.isfinite(t)] = np.nan
    raw.setflags(write=False)
    return raw, a, np.tile(np.arange(len(el)), n_az)


def set_azimuth(raw, rows, ori):
    """Turn rows about the z axis to azimuth `ori`: range and elevation (the ring) stay."""
    rho = np.hypot(raw[rows, 0].astype(np.float64), raw[rows, 1].astype(np.float64))
    raw[rows, 0] = rho * np.cos(ori)
    raw[rows, 1] = -rho * np.sin(ori)


def put_point(raw, row, ori, rho, elev_deg):
    raw[row] = ring_rows([ori], [rho], [elev_deg])[0]


def wrap(a):
    return (np.asarray(a, np.float64) + PI) % (2 * PI) - PI


# ------------------------------------------------------------------------------------------------
# numpy model 1: start / end azimuth, latch, wrap branches, relTime (lo_extract.cpp:123-171)
# ------------------------------------------------------------------------------------------------
def kept_by_filters(raw, near_range):
    x, y, z = raw[:, 0], raw[:, 1], raw[:, 2]
    with np.errstate(invalid="ignore"):
        thres = np.float32(near_range)
        return np.isfinite(x) & np.isfinite(y) & np.isfinite(z) & ~((x * x + y * y + z * z) < thres * thres)


def azimuth_logic(ori, start, end_raw, T):
    """ori: azimuth of every ring-valid point in firing order (type T), start: startOri, end_raw: -atan2(last) before + 2 pi.  Sums and comparisons against
    multiples of pi in f64, stores narrowed to T — as the reference's mixed float / double expressions.  -> dict."""
    f = np.float64
    ori = np.asarray(ori, T)
    end = T(f(end_raw) + 2 * PI)
    corr = "none"
    if f(T(end - start)) > 3 * PI:
        end, corr = T(f(end) - 2 * PI), "minus"
    elif f(T(end - start)) < PI:
        end, corr = T(f(end) + 2 * PI), "plus"
    a1 = ori.astype(f) < f(start) - PI / 2
    a2 = ~a1 & (ori.astype(f) > f(start) + PI * 3 / 2)
    o1 = np.where(a1, (ori.astype(f) + 2 * PI).astype(T), np.where(a2, (ori.astype(f) - 2 * PI).astype(T), ori)).astype(T)
    latch = (o1 - start).astype(T).astype(f) > PI
    pos = int(np.argmax(latch)) if latch.any() else None
    first = np.ones(ori.shape[0], bool) if pos is None else np.arange(ori.shape[0]) <= pos
    o2 = (ori.astype(f) + 2 * PI).astype(T)
    b1 = o2.astype(f) < f(end) - PI * 3 / 2
    b2 = ~b1 & (o2.astype(f) > f(end) + PI / 2)
    o2 = np.where(b1, (o2.astype(f) + 2 * PI).astype(T), np.where(b2, (o2.astype(f) - 2 * PI).astype(T), o2)).astype(T)
    o = np.where(first, o1, o2).astype(T)
    rel = ((o - start).astype(T) / T(end - start)).astype(T)
    return dict(corr=corr, latch_pos=pos, A1=int((a1 & first).sum()), A2=int((a2 & first).sum()), B1=int((b1 & ~first).sum()), B2=int((b2 & ~first).sum()),
                rel_min=float(rel.min()) if rel.size else 0.0, rel_max=float(rel.max()) if rel.size else 0.0, rel=rel, start=float(start), end=float(end))


def azimuth_model(c, full_src, T=np.float32):
    """The model on the scan itself: full_src = the oracle's list of surviving rows (NaN, near range and the ring table)."""
    raw = c["raw"]
    ok = np.nonzero(kept_by_filters(raw, c["near_range"]))[0]
    first, last = ok[0], ok[-1]
    at2 = lambda r: (-np.arctan2(raw[r, 1].astype(T), raw[r, 0].astype(T))).astype(T)      # noqa: E731
    rows = np.sort(np.asarray(full_src))
    m = azimuth_logic(at2(rows), T(at2(first)), T(at2(last)), T)
    m["half_idx"] = INT_MAX if m["latch_pos"] is None else int(rows[m["latch_pos"]])
    m["rows"] = rows
    return m


def design_claim(ori_rows, valid_rows):
    """The same logic in f64 on the DESIGNED azimuths (what the builder asked for, not what the stored float32 coordinates give): ori_rows = azimuth per row,
    valid_rows = rows the design keeps (on the ring table, a return)."""
    o = wrap(ori_rows)
    v = np.asarray(valid_rows)
    m = azimuth_logic(o[v], np.float64(o[v[0]]), np.float64(o[v[-1]]), np.float64)
    m["half_idx"] = INT_MAX if m["latch_pos"] is None else int(v[m["latch_pos"]])
    return {k: m[k] for k in ("corr", "half_idx", "A1", "A2", "B1", "B2", "rel_min", "rel_max")}


# ------------------------------------------------------------------------------------------------
# numpy model 2: one segment's greedy run (lo_extract.cpp:211-240), float32 gaps and ranges
# ------------------------------------------------------------------------------------------------
def gap2(cloud, a, b):
    d = cloud[a, :3] - cloud[b, :3]
    return np.float32(np.float32(d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])


def range2(cloud, k):
    p = cloud[k, :3]
    return np.float32(np.float32(p[0] * p[0] + p[1] * p[1]) + p[2] * p[2])


def break_offset(cloud, ind, sign):
    """The l in 1 .. 5 at which the suppression loop of a pick at `ind` stops in direction `sign`, or None."""
    for l in range(1, 6):
        if float(gap2(cloud, ind + sign * l, ind + sign * (l - 1))) > GAP_BREAK:
            return l
    return None


def _suppress(cloud, picked, ind):
    picked[ind] = 1
    for s in (1, -1):
        b = break_offset(cloud, ind, s)
        for l in range(1, (b if b is not None else 6)):
            picked[ind + s * l] = 1


def greedy_segment(cloud, curv, sp, ep, picked, near_check=True):
    """picked: the mark array over the whole cloud as the segment finds it (modified in place).  -> (edge picks in push order, flat picks in push order)."""
    order = sp + np.argsort(curv[sp:ep + 1], kind="stable")
    edge, flat = [], []
    n = 0
    for ind in order[::-1]:
        if picked[ind] == 0 and float(curv[ind]) > CURV_SHARP:
            n += 1
            if n > 10:
                break
            edge.append(int(ind))
            _suppress(cloud, picked, ind)
    n = 0
    for ind in order:
        if near_check and float(range2(cloud, ind)) < 0.25:
            continue
        if picked[ind] == 0 and float(curv[ind]) < CURV_FLAT:
            flat.append(int(ind))
            n += 1
            if n >= 4:
                break
            _suppress(cloud, picked, ind)
    return edge, flat


def ring_serial(o, ring, near_check=True):
    """The six segments of one ring of the oracle's result in the reference's order -> per segment (edge, flat, marks as the segment found them)."""
    cloud, curv = o["full"], o["curvature"]
    rs, re = int(o["ring_start"][ring]), int(o["ring_end"][ring])
    picked = np.zeros(cloud.shape[0] + 8, np.int8)
    out = []
    for j in range(6):
        sp, ep = rs + (re - rs) * j // 6, rs + (re - rs) * (j + 1) // 6 - 1
        before = picked.copy()
        e, f = greedy_segment(cloud, curv, sp, ep, picked, near_check)
        out.append(dict(sp=sp, ep=ep, edge=e, flat=f, marks_in=before))
    return out


def segment_alone(o, ring, j, marks_in=None):
    """Segment j of a ring run on its own: without incoming marks (what a concurrent segment does first), or with the given ones."""
    rs, re = int(o["ring_start"][ring]), int(o["ring_end"][ring])
    sp, ep = rs + (re - rs) * j // 6, rs + (re - rs) * (j + 1) // 6 - 1
    picked = np.zeros(o["full"].shape[0] + 8, np.int8) if marks_in is None else marks_in.copy()
    e, f = greedy_segment(o["full"], o["curvature"], sp, ep, picked)
    return dict(sp=sp, ep=ep, edge=e, flat=f, marks_out=picked)


def voxel_coords(xyz, ds_v):
    """floor(coordinate / leaf) as k_rot_scatter and pcl::VoxelGrid form it: float32 product with the float32 inverse leaf."""
    inv = np.float32(1.0) / np.float32(ds_v)
    return np.floor(np.asarray(xyz, np.float32) * inv).astype(np.int64)


# ------------------------------------------------------------------------------------------------
# family: sweep
# ------------------------------------------------------------------------------------------------
SWEEP_STARTS = (0.8, 2.4, -2.4, -0.8, 3.1, -3.1)          # every quadrant, both sides of +-pi
SWEEPS = (("0.4pi", 0.4 * PI), ("pi-", PI - 0.05), ("pi+", PI + 0.05), ("2pi", 2 * PI), ("2.6pi", 2.6 * PI))


def _valid_rows(raw, ring, n_scans=64):
    """Rows the design keeps: a return, farther than 3 m, on the ring table (ids above 50 of the 64-ring table are dropped)."""
    return np.nonzero(kept_by_filters(raw, 3.0) & (ring <= (50 if n_scans == 64 else n_scans - 1)))[0]


def _sweep_case(name, family, start, sweep, n_az=201, elev="hdl64", edit=None, **kw):
    raw, ori, ring = scene_scan(start, sweep, n_az, elev, scene="room")
    raw, ori = raw.copy(), ori.copy()
    if edit:
        edit(raw, ori, ring)
    claim = design_claim(ori, _valid_rows(raw, ring))
    claim.update(start=start, sweep=sweep)
    return case(name, family, raw, claim=claim, q_imu=Q_SMALL, q_lb=Q_LB, ds_rate=4, **kw)


def _move_steps(steps, to, only=None):
    """Edit: the rows of the given azimuth steps (of the rings in `only`) are turned to azimuth `to` (+ 1 mrad per step: no two rows coincide)."""
    def edit(raw, ori, ring):
        per = int(ring.max()) + 1
        for s in steps:
            rows = np.arange(s * per, (s + 1) * per)
            if only is not None:
                rows = rows[np.isin(ring[rows], only)]
            rows = rows[np.isfinite(raw[rows, 0])]
            set_azimuth(raw, rows, to + 1e-3 * (s - steps[0]))
            ori[rows] = to + 1e-3 * (s - steps[0])
    return edit


def sweep_cases():
    out = []
    for s in SWEEP_STARTS:
        for tag, sw in SWEEPS:
            out.append(_sweep_case(f"sweep_{s:+.1f}_{tag}", "sweep", s, sw))
    # a block fired BEFORE the start azimuth (by 0.8 rad) early in the scan: `ori > startOri + 3 pi / 2` once wrapped
    out.append(_sweep_case("sweep_block_before_start", "sweep", -2.4, 2 * PI, edit=_move_steps((10, 11, 12), -2.4 - 0.8)))
    # a block of the first quarter fired late in the second half: `ori + 2 pi < endOri - 3 pi / 2`
    out.append(_sweep_case("sweep_block_early_late", "sweep", 2.4, 2 * PI, edit=_move_steps((170, 171, 172), 2.4 + 1.0)))
    return out


# ------------------------------------------------------------------------------------------------
# family: latch (51 rows per step: row 1023 is ring 3 of step 20, row 1024 ring 4)
# ------------------------------------------------------------------------------------------------
LATCH_STEPS = 381                                          # 19 431 rows: the last workgroup of 1024 starts at row 18 432
LATCH_LAST_ROW = 18 * 1024 + 57


def _stray(row, start):
    def edit(raw, ori, ring):
        put_point(raw, row, start + PI + 0.3, 20.0, ELEV64[ring[row]])
        ori[row] = start + PI + 0.3
    return edit


def latch_cases():
    s = 0.8
    out = [_sweep_case("latch_none", "latch", s, 0.9 * PI, LATCH_STEPS, "ids51"),
           _sweep_case("latch_last_workgroup", "latch", s, 0.9 * PI, LATCH_STEPS, "ids51", edit=_stray(LATCH_LAST_ROW, s)),
           _sweep_case("latch_natural", "latch", s, 2 * PI, LATCH_STEPS, "ids51"),
           _sweep_case("latch_row_1023", "latch", s, 2 * PI, LATCH_STEPS, "ids51", edit=_stray(1023, s)),
           _sweep_case("latch_row_1024", "latch", s, 2 * PI, LATCH_STEPS, "ids51", edit=_stray(1024, s))]
    for c, want in zip(out, (INT_MAX, LATCH_LAST_ROW, None, 1023, 1024)):
        c["claim"]["half_idx_by_hand"] = want
    assert out[0]["raw"].shape[0] == 51 * LATCH_STEPS and LATCH_LAST_ROW // 1024 == (out[0]["raw"].shape[0] - 1) // 1024
    return out


# ------------------------------------------------------------------------------------------------
# family: reltime
# ------------------------------------------------------------------------------------------------
def reltime_cases():
    s = 0.8
    out = [_sweep_case("reltime_neg_ring0", "reltime", s, 2 * PI, edit=_move_steps(tuple(range(10, 40)), s - 0.3, only=[0])),
           _sweep_case("reltime_neg_rings", "reltime", s, 2 * PI, edit=_move_steps((10, 11), s - 0.3, only=list(range(1, 51)))),
           _sweep_case("reltime_ge1", "reltime", s, 2 * PI, edit=_move_steps((180, 181), s + 0.3))]
    # by hand: relTime = (azimuth - start) / span, span = 2 pi (1 - 1 / 201); the last step's points define endOri: theirs is 1
    out[0]["claim"].update(by_hand=dict(rel_min=(-0.06, -0.04), rel_max=(0.9, 1.000001), neg_rings="zero"))
    out[1]["claim"].update(by_hand=dict(rel_min=(-0.06, -0.04), rel_max=(0.9, 1.000001), neg_rings="positive"))
    out[2]["claim"].update(by_hand=dict(rel_min=(0.0, 0.0), rel_max=(1.04, 1.06), neg_rings=None))
    return out


# ------------------------------------------------------------------------------------------------
# family: tables
# ------------------------------------------------------------------------------------------------
def table_id(angle, n_scans):
    """Ring id of an elevation in degrees, or -1 (lo_extract.cpp:148-159), in f64 on the DESIGNED angle."""
    a = float(angle)
    if n_scans == 16:
        i = int((a + 15) / 2 + 0.5)
        return i if 0 <= i <= 15 else -1
    if n_scans == 32:
        i = int((a + 92.0 / 3.0) * 3.0 / 4.0)
        return i if 0 <= i <= 31 else -1
    i = int((2 - a) * 3.0 + 0.5) if a >= -8.83 else 32 + int((-8.83 - a) * 2.0 + 0.5)
    return -1 if (a > 2 or a < -24.33 or i > 50 or i < 0) else i


def table_boundaries(n_scans):
    """Every elevation at which the ring id changes or a point starts to be dropped."""
    if n_scans == 16:
        return [2.0 * k - 16.0 for k in range(-1, 17)]                       # int() truncates towards zero: id 0 reaches down to -18
    if n_scans == 32:
        return [-92.0 / 3.0 + 4.0 * k / 3.0 for k in range(-1, 33)]          # id 0 reaches down to -32
    up = [2.0 - (k - 0.5) / 3.0 for k in range(1, 33)]
    low = [-8.83 - (m - 0.5) / 2.0 for m in range(1, 20)]                    # m = 19: scanID 50 | 51 at -18.08
    return up + low + [2.0, -8.83, -24.33]


def tables_cases():
    out = []
    for n_scans in (16, 32, 64):
        b = np.array(table_boundaries(n_scans))
        ang = np.concatenate([b - 0.02, b + 0.02, [40.0, 25.0, -40.0, -55.0]])
        n_az = 150
        ori = 0.4 + 2 * PI * np.arange(n_az) / n_az
        a, e = np.repeat(ori, ang.shape[0]), np.tile(ang, n_az)
        rng = np.random.default_rng(16 + n_scans)
        rho = 15.0 + 5.0 * np.cos(3 * a) + rng.uniform(-2e-3, 2e-3, a.shape)
        raw = ring_rows(a, rho, e, refl=rng.integers(1, 255, a.shape[0]))
        ids = np.array([table_id(v, n_scans) for v in ang])
        out.append(case(f"tables_{n_scans}", "tables", raw, n_scans=n_scans, q_imu=Q_SMALL, q_lb=Q_LB,
                        claim=dict(ids=np.tile(ids, n_az), n_dropped=int((ids < 0).sum()) * n_az, ids_hit=sorted(set(ids[ids >= 0].tolist())))))
    return out


# ------------------------------------------------------------------------------------------------
# family: sizes
# ------------------------------------------------------------------------------------------------
def _room_ring(n, elev_deg, seed, start=0.3, half=30.0):
    ori = start + 2 * PI * np.arange(n) / max(n, 1)
    rng = np.random.default_rng(seed)
    return ring_rows(ori, room_rho(ori, elev_deg, half) + rng.uniform(-2e-2, 2e-2, n), elev_deg, refl=rng.integers(1, 255, n))


RING_COUNTS = (0, 5, 11, 16, 17, 74, 75, 300, 6, 12, 18, 73, 76, 1, 10, 64)


def sizes_cases():
    out = []
    base = scene_scan(0.8, 2 * PI, 200, "hdl64")[0]
    for n in (1, 1023, 1024, 1025):
        out.append(case(f"sizes_n{n}", "sizes", base[:n], q_imu=Q_SMALL, q_lb=Q_LB, claim=dict(rows=n)))
    # more rows than one trip of the histogram sum takes, every ring within the LDS working set: 51 rings x 4000 steps + 15 dropped rows per step
    n_az, el = 4000, ELEV64[:51]
    ori = 0.3 + 2 * PI * np.arange(n_az) / n_az
    rng = np.random.default_rng(77)
    blk = np.full((n_az, 66, 4), 10.0, np.float32)
    for r, e in enumerate(el):
        blk[:, r] = ring_rows(ori, room_rho(ori, e) + rng.uniform(-2e-2, 2e-2, n_az), e, refl=rng.integers(1, 255, n_az))
    blk[:, 51:56, 0] = np.nan                                                                   # no return
    blk[:, 56:61] = ring_rows(np.repeat(ori, 5), np.full(5 * n_az, 0.5), np.zeros(5 * n_az)).reshape(n_az, 5, 4)      # inside the near range
    blk[:, 61:66] = ring_rows(np.repeat(ori, 5), np.full(5 * n_az, 20.0), np.full(5 * n_az, 10.0)).reshape(n_az, 5, 4)   # above the 64-ring table
    out.append(case("sizes_two_trips", "sizes", blk.reshape(-1, 4), ds_rate=4, q_imu=Q_SMALL, q_lb=Q_LB,
                    claim=dict(rows=66 * n_az, max_ring=n_az, n_full=51 * n_az)))
    # ring lengths at the thresholds: fewer than 12 points (ring_end < ring_start), 16 | 17 (`re - rs < 6`), 74 | 75 (segments of 64 points run concurrently)
    rings = [_room_ring(c, TABLE16[r], 300 + r) for r, c in enumerate(RING_COUNTS)]
    out.append(case("sizes_ring_counts", "sizes", interleave(rings), n_scans=16, claim=dict(ring_counts=list(RING_COUNTS), rows=sum(RING_COUNTS))))
    # rings of exactly the LDS working set and one more, beside ordinary rings: the second pass runs over a partly finished scan
    counts = [1800] * 16
    counts[2], counts[4], counts[11] = LDS_CAP, LDS_CAP + 1, LDS_CAP
    rings = [_room_ring(c, TABLE16[r], 2800 + r) for r, c in enumerate(counts)]      # (seeds of the noise: chosen so that no two curvatures of a segment are equal)
    out.append(case("sizes_lds_boundary", "sizes", interleave(rings), n_scans=16, claim=dict(ring_counts=counts, rows=sum(counts), mixed=True)))
    # one ring whose SEGMENTS are longer than the LDS working set
    n = 6 * LDS_CAP + 24
    out.append(case("sizes_single_ring", "sizes", _room_ring(n, TABLE16[8], 501), n_scans=16,
                    claim=dict(ring_counts=[n if r == 8 else 0 for r in range(16)], rows=n, min_segment=LDS_CAP + 1)))
    return out


# ------------------------------------------------------------------------------------------------
# polyline rings (picks, borders): one ring of the 16-ring table at +1 deg, a circle of 10 m with 1 mm jitter and radial spikes
# ------------------------------------------------------------------------------------------------
POLY_N, POLY_RING, POLY_RHO = 1200, 8, 10.0


def poly_ring(spikes, n=POLY_N, seed=0, jitter=1e-3, dori=None, rho_edit=None):
    """spikes: {ring-local index: height}.  dori: {index k: tangential distance between points k - 1 and k} replacing the regular step.  rho_edit(rho)."""
    rng = np.random.default_rng(2000 + seed)
    rho = POLY_RHO + jitter * rng.uniform(-1, 1, n)
    step = np.full(n, 2 * PI / n)
    for k, dist in (dori or {}).items():
        step[k] = dist / POLY_RHO
    ori = 0.2 + np.cumsum(step) - step[0]
    if rho_edit:
        rho_edit(rho)
    for k, h in spikes.items():
        rho[k] += h
    return ring_rows(ori, rho, TABLE16[POLY_RING], refl=rng.integers(1, 255, n))


def _seg(j, n=POLY_N):
    return segment_bounds(n, j)


def picks_cases():
    out = []
    # 2, 10 and 12 eligible candidates (curvature > 2) in segments 0, 1, 2
    spikes, want = {}, {}
    for j, cnt in ((0, 2), (1, 10), (2, 12)):
        sp, _ = _seg(j)
        for m in range(cnt):
            spikes[sp + 9 + 14 * m] = 0.170 + 0.003 * ((5 * m) % 12)
        want[j] = cnt
    out.append(case("picks_counts", "picks", poly_ring(spikes, seed=1), n_scans=16, claim=dict(eligible=want, spikes=sorted(spikes))))

    # flat picks in a designed order: over the first points of segment 0 the range grows with the cube of the index, so the curvature grows with the index — picks at
    # +0, +6, +12 (each marks five points either side), the next candidate in the order (+13) lies under the third pick's marks, the fourth pick is +18
    sp0, _ = _seg(0)

    def cubic(rho):
        k = np.arange(rho.shape[0])
        t = np.clip(k - sp0, 0, 40).astype(np.float64)
        rho[:] = POLY_RHO - 1e-5 * t ** 3          # (inwards: the same sign as the circle's own second difference)
        rest = k > sp0 + 40
        rho[rest] += 0.6                                                      # a step between the two: curvatures (0.6 m)^2 with m = 1 .. 5 points beyond it
        rho[rest] += 0.05 * np.where(k[rest] % 2 == 0, 1.0, -1.0)             # the rest of the ring: a zigzag, curvature 144 * 0.05^2 = 0.36 — not flat
        rho[rest] += 1e-3 * np.random.default_rng(31).uniform(-1, 1, int(rest.sum()))      # (no two curvatures equal)
    out.append(case("picks_flat_fourth", "picks", poly_ring({}, seed=2, jitter=0.0, rho_edit=cubic), n_scans=16,
                    claim=dict(flat_seg0=[sp0, sp0 + 6, sp0 + 12, sp0 + 18], skipped=sp0 + 13)))

    # squared gaps 3 % above and 3 % below 0.05 at l = +-1 .. +-5 from a pick: 20 spikes of 0.19 m, each with ONE widened step beside it
    h = 0.19
    spikes, dori, want = {}, {}, []
    slot = 0
    for l in (1, 2, 3, 4, 5, -1, -2, -3, -4, -5):
        for side, g2 in (("above", 0.0515), ("below", 0.0485)):
            j, m = divmod(slot, 4)
            p = _seg(j)[0] + 30 + 40 * m
            slot += 1
            spikes[p] = h
            k = p + l if l > 0 else p + l + 1                                    # the step between points k - 1 and k is the one the loop tests at offset l
            dori[k] = float(np.sqrt(g2 - (h * h if abs(l) == 1 else 0.0)))
            want.append((p, l, side))
    out.append(case("picks_gaps", "picks", poly_ring(spikes, seed=3, jitter=2e-4, dori=dori), n_scans=16, claim=dict(gaps=want)))

    # ten separated spikes in every segment: 60 edge, 12 sharp and 24 flat picks on one ring (the field maxima of the ring's fold word)
    spikes = {}
    for j in range(6):
        sp, _ = _seg(j)
        for m in range(10):
            spikes[sp + 9 + 18 * m] = 0.170 + 0.003 * ((7 * m + j) % 12)
    out.append(case("picks_caps", "picks", poly_ring(spikes, seed=4), n_scans=16, claim=dict(caps=(60, 12, 24))))
    return out


def borders_cases():
    out = []
    for j in (1, 5):
        sp, _ = _seg(j)
        out.append(case(f"borders_hit_j{j}", "borders", poly_ring({sp - 2: 0.20, sp + 3: 0.18}, seed=10 + j), n_scans=16,
                        claim=dict(hit=[(j, sp + 3)], not_hit=[])))
    # chain: B (first five of segment 2) lies under A's marks; with B segment 2 holds eleven candidates and D, its smallest, is cut by the limit of ten;
    # without B (the redo) D is picked and ITS marks reach E in the first five of segment 3
    sp2, ep2 = _seg(2)
    sp3, _ = _seg(3)
    assert sp3 == ep2 + 1
    spikes = {sp2 - 2: 0.20, sp2 + 3: 0.203, sp3 - 3: 0.170, sp3 + 2: 0.19}
    for m in range(9):
        spikes[sp2 + 20 + 17 * m] = 0.175 + 0.003 * m
    out.append(case("borders_chain", "borders", poly_ring(spikes, seed=13), n_scans=16, claim=dict(hit=[(2, sp2 + 3)], chain=(3, sp3 + 2), not_hit=[])))
    # a pick in the first five that is NOT hit: the spike before the border is 0.25 m high — the gap beside it breaks the suppression at l = 1
    sp, _ = _seg(4)
    out.append(case("borders_not_hit", "borders", poly_ring({sp - 2: 0.25, sp + 3: 0.18}, seed=14), n_scans=16, claim=dict(hit=[], not_hit=[(4, sp + 3)])))
    return out


# ------------------------------------------------------------------------------------------------
# family: near  (near_range 0.1: the `range2 < 0.25` branch of the flat loop, the less-flat list and the voxel candidates)
# ------------------------------------------------------------------------------------------------
def near_cases():
    n = 480
    ori = 0.2 + 1.0 * np.arange(n) / n
    rings = []
    for r in range(16):
        rng = np.random.default_rng(600 + r)
        rho = np.where((np.arange(n) // 40) % 2 == 0, 0.40, 0.55) + 2e-4 * rng.uniform(-1, 1, n)      # 0.4 m: range^2 < 0.25 on every ring; 0.55 m: > 0.3
        rings.append(ring_rows(ori, rho, TABLE16[r], refl=rng.integers(1, 255, n)))
    return [case("near_half_metre", "near", interleave(rings), n_scans=16, near_range=0.1, claim=dict(min_near=20, min_flat_otherwise=5))]


# ------------------------------------------------------------------------------------------------
# family: voxels
# ------------------------------------------------------------------------------------------------
VOX_EDGE_LEAF = 0.1            # packed key: 11 | 11 | 9 bits -> x, y in [-102.4, 102.4), z in [-25.6, 25.6)


def _vox_edge_scan(one_past):
    n_az = 400
    ori = 0.3 + 2 * PI * np.arange(n_az) / n_az
    rng = np.random.default_rng(88)
    blk = np.empty((n_az, 16, 4), np.float32)
    for r in range(16):
        blk[:, r] = ring_rows(ori, 50.0 + rng.uniform(-5e-3, 5e-3, n_az), TABLE16[r], refl=rng.integers(1, 255, n_az))
    T = 102.35                      # floor(102.35 / 0.1) = 1023, floor(-102.35 / 0.1) = -1024: the last packed coordinates

    def far(target_ori, horizontal, r=8):
        s = int(np.argmin(np.abs(wrap(ori - target_ori))))
        c = abs(np.cos(ori[s])) if abs(np.cos(target_ori)) > 0.5 else abs(np.sin(ori[s]))
        blk[s, r] = ring_rows([ori[s]], [horizontal / c], [TABLE16[r]])[0]
    far(0.0, T); far(PI, T); far(-PI / 2, T); far(PI / 2, T)
    zr = 25.55 / np.tan(np.deg2rad(15.0))
    far(PI / 4, zr * np.cos(ori[int(np.argmin(np.abs(wrap(ori - PI / 4))))]), r=15)           # z = +25.55: floor = 255
    far(3 * PI / 4, zr * abs(np.cos(ori[int(np.argmin(np.abs(wrap(ori - 3 * PI / 4))))])), r=0)   # z = -25.55: floor = -256
    if one_past:
        far(0.1, 102.45, r=6)       # floor(102.45 / 0.1) = 1024
    return blk.reshape(-1, 4)


def voxels_cases():
    out = []
    # a ring that alternates between two voxels point by point: every candidate its own run, 1500 equal keys per voxel
    n = 3000
    ori = 0.001 + 0.029 * np.arange(n) / n
    rho = np.where(np.arange(n) % 2 == 0, 10.15, 10.25)            # x = 10.2 = 17 * 0.6 lies between: curvature (6 * 0.1)^2, no pick at all
    out.append(case("voxels_alternating", "voxels", ring_rows(ori, rho, TABLE16[POLY_RING]), n_scans=16, claim=dict(n_voxels=2, min_runs=2900), ref=False))
    # spikes of 0.7 m: each leaves the voxels of the circle, is picked as an edge and so leaves the less-flat list — its voxel has no centroid
    spikes = {_seg(j)[0] + 90: 0.7 for j in range(6)}
    out.append(case("voxels_all_picked", "voxels", poly_ring(spikes, seed=20), n_scans=16, claim=dict(spikes=sorted(spikes))))
    out.append(case("voxels_last_key", "voxels", _vox_edge_scan(False), n_scans=16, ds_v=VOX_EDGE_LEAF, claim=dict(overflow=0)))
    out.append(case("voxels_one_past", "voxels", _vox_edge_scan(True), n_scans=16, ds_v=VOX_EDGE_LEAF, claim=dict(overflow=1)))
    base = scene_scan(0.8, 2 * PI, 600, "vlp16")[0]
    for ds in (3, 5, 17):
        out.append(case(f"voxels_ds_rate_{ds}", "voxels", base, n_scans=16, ds_rate=ds, q_imu=Q_SMALL, q_lb=Q_LB,
                        claim=dict(rings=[r for r in range(16) if r % ds == 0])))
    return out


# ------------------------------------------------------------------------------------------------
# family: ties
# ------------------------------------------------------------------------------------------------
def ties_cases():
    # z = 0 on the 64-ring table: (2 - 0) * 3 + 0.5 = 6.5 -> ring 6, in the middle of its bin.  x = -4 + k / 128, y = 8 (+ 0.25): every coordinate exact in float32
    n = 1025
    k = np.arange(n)
    line = np.zeros((n, 4), np.float32)
    line[:, 0] = -4.0 + k / 128.0
    line[:, 1] = 8.0
    line[:, 3] = 10.0
    spiked = line.copy()
    spiked[k % 12 == 6, 1] = 8.25
    return [case("ties_collinear", "ties", line, claim=dict(min_ties=900, all_zero=True), ref=False),
            case("ties_equal_spikes", "ties", spiked, claim=dict(min_ties=500, spike_curv=6.25), ref=False)]


# ------------------------------------------------------------------------------------------------
# family: slerp
# ------------------------------------------------------------------------------------------------
SLERP_Q = {
    "identity": IDENTITY,
    "negated": tuple(-v for v in Q_SMALL),                                                   # w < 0
    "three_rad": (np.cos(1.5), 0.6 * np.sin(1.5), -0.3 * np.sin(1.5), np.sqrt(1 - 0.36 - 0.09) * np.sin(1.5)),
    "one_ulp_below_one": (float(np.nextafter(1.0, 0.0)), 1e-9, -2e-9, 1e-9),                 # |w| >= 1 - 2.2e-16: qslerp_prepare's linear branch
}


def slerp_cases():
    base = scene_scan(0.8, 2 * PI, 200, "hdl64")[0]
    out = []
    for qn, q in SLERP_Q.items():
        for ln, qlb in (("qlb", Q_LB), ("unit", IDENTITY)):
            out.append(case(f"slerp_{qn}_{ln}", "slerp", base, ds_rate=4, q_imu=q, q_lb=qlb, claim=dict(q=qn)))
    return out


@functools.lru_cache(maxsize=None)
def all_cases():
    out = sweep_cases() + latch_cases() + reltime_cases() + tables_cases() + sizes_cases() + picks_cases() + borders_cases() + near_cases() + voxels_cases() \
        + ties_cases() + slerp_cases()
    assert len({c["name"] for c in out}) == len(out)
    for c in out:
        c["raw"].setflags(write=False)
    return tuple(out)


def cases_of(*families):
    return [c for c in all_cases() if c["family"] in families]


def by_name(name):
    return next(c for c in all_cases() if c["name"] == name)
