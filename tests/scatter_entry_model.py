"""A binary64 model of the hash grid's table gradient, PER TABLE ELEMENT, and the error bound every scatter route of
csrc/hashgrid.hip owes it (test infrastructure: plain numpy, no GPU).

The table gradient of include/mi3d.h Part 2 / Part 3 is, for table element (level l, entry e, feature f),

    grad[l, e, f] = sum over the contributions (point q, corner k) with entry(q, l, k) == e of  w(q, l, k) * d(q, l, f)

with w the binary32 trilinear weight and entry the lattice rule `oracle.hashgrid_indices` returns (the cells are bit-exact
by contract, tests/test_hashgrid_gpu.py::test_level_table_matches_oracle pins the scales) and d the feature gradient of
the point.  `entry_model` evaluates that sum with products and additions in binary64 (`ref`) and keeps, per element, what
an error bound needs: A = sum |w d|, m = the number of non-zero contributions, B = sum |d| over them; per level the
largest |d|, the largest A and the largest m.  `entry_bound` turns them into the bound of one route, `check_entries`
compares a kernel's result with it element by element - every element of every level, no quantile, no global maximum.
"""
import numpy as np

U = 2.0 ** -24          # unit roundoff of binary32

# Roundings INSIDE one contribution, per route (the `c` of entry_bound); see entry_bound's docstring for the derivation.
# ("single": a fine level that cannot pair - more than 2^19 entries - which only a grid with log2_hashmap_size 20 and more
# has; tests/test_scatter_entry_gpu.py reaches it with such a grid.)
ROUTE_C = {"atomic": 1, "pair": 6, "single": 2, "coarse": 3}
RECORD_ROUTES = ("pair", "single", "coarse")
TERMS = ("binary32", "reduce", "gather", "rec16")


class EntryModel:
    def __init__(self, cfg):
        self.cfg = cfg
        n = cfg.n_params
        self.ref, self.A, self.B = np.zeros(n), np.zeros(n), np.zeros(n)
        self.m = np.zeros(n, np.int64)
        self.dmax = np.zeros(cfg.n_levels)      # largest |d| of a contributing point, per level
        self.has_extra = False

    def level_slice(self, l):
        return slice(int(self.cfg.offsets[l]) * 2, int(self.cfg.offsets[l + 1]) * 2)

    def add(self, oracle, x01, grad):
        """One point set: x01 [n, 3] binary32 in [0, 1], grad [n, L, 2] binary32 or binary16 (taken at its own values) - or a
        stack [K, n, L, 2] of K gradients at the SAME positions (the 13 coinciding points of the overflow case, point 0 and
        its extra pair): K contributions per corner, with the lattice looked up once.  (The K products of a corner are then
        summed as w * sum d: one binary64 rounding of a sum of at most 16 numbers, 2^-29 of the binary32 unit.)"""
        cfg = self.cfg
        x01 = np.ascontiguousarray(x01, np.float32).reshape(-1, 3)
        n, L = x01.shape[0], cfg.n_levels
        d = np.asarray(grad).reshape(-1, n, L, 2).astype(np.float64)
        assert d.shape[0] <= 16
        dsum, dabs, cnt = d.sum(0), np.abs(d).sum(0), (d != 0).sum(0)            # [n, L, 2]
        idx, w = oracle.hashgrid_indices(x01, cfg)                               # [n, L, 8] entries, binary32 weights
        flat = (idx.astype(np.int64) + cfg.offsets[:L].astype(np.int64)[None, :, None]) * 2
        flat = np.stack([flat, flat + 1], -1).reshape(-1)                        # [n, L, 8, 2] -> table elements
        w = np.broadcast_to(w.astype(np.float64)[..., None], (n, L, 8, 2)).reshape(-1)
        live = (w != 0) & (np.broadcast_to(cnt[:, :, None, :], (n, L, 8, 2)).reshape(-1) != 0)
        flat, w = flat[live], w[live]

        def per_corner(a):
            return np.broadcast_to(a[:, :, None, :], (n, L, 8, 2)).reshape(-1)[live]
        N = cfg.n_params
        self.ref += np.bincount(flat, w * per_corner(dsum), N)                   # (K = 1: exact, 24 x 24 bits)
        self.A += np.bincount(flat, w * per_corner(dabs), N)
        self.B += np.bincount(flat, per_corner(dabs), N)
        self.m += np.bincount(flat, per_corner(cnt), N).astype(np.int64)
        self.dmax = np.maximum(self.dmax, np.abs(d).max(axis=(0, 1, 3)) if n else 0.0)
        return self

    def finish(self):
        L = self.cfg.n_levels
        self.Amax = np.array([self.A[self.level_slice(l)].max() for l in range(L)])
        self.mmax = np.array([self.m[self.level_slice(l)].max() for l in range(L)])
        for a in (self.ref, self.A, self.B, self.m, self.dmax, self.Amax, self.mmax):
            a.setflags(write=False)
        return self


def entry_model(oracle, cfg, x01_sets, grad_sets, extra0=None):
    """The model of one scatter call: `x01_sets[p]` [n, 3] and `grad_sets[p]` [n, L, 2] for every stencil point p, and
    optionally `extra0` = the second gradient pair of point 0 ([n, L, 2], at x01_sets[0]'s positions): to the model it is
    one more point set - w (a + b) = w a + w b exactly - and what a route does with it is entry_bound's business."""
    mdl = EntryModel(cfg)
    for x01, g in zip(x01_sets, grad_sets):
        mdl.add(oracle, x01, g)
    if extra0 is not None:
        mdl.add(oracle, x01_sets[0], extra0)
        mdl.has_extra = True
    return mdl.finish()


def entry_bound(mdl, routes, half=False, extra_summed=False):
    """The error bound of every table element, as a dict of its terms (arrays over the table) plus "total" and the
    constants used ("c": per level).  `routes[l]` names what level l goes through:

      "atomic"  k_scatter / k_scatter_runs (+ k_replica_reduce): float atomics, straight or run-merged first
      "pair"    k_bin_emit's fine role: x-pair records (16 bytes; 12 bytes with binary16 planes: `half`) -> k_bin_reduce
      "single"  k_bin_emit's fine role on a level that cannot pair: one 12-byte record per contribution -> k_bin_reduce
      "coarse"  k_bin_emit's coarse role: register sums, the wave's LDS gather table, one record per entry -> k_bin_reduce
    `extra_summed`: the call carries the extra point-0 pair AND this route adds it to point 0's pair in binary32 before
    anything else (fp32 planes on "pair" / "single", both plane types on "coarse"; binary16 pair records carry it as a
    record of its own, the atomic routes scatter it in a pass of its own: not summed).

    Derivation (u = 2^-24; every constant from include/mi3d.h Part 3 and the comments of hashgrid.hip, none from output):

    BINARY32 TERM, every route: (m + c) u A.  The result is a sum of m products.  Whatever the order - atomics in
    arrival order, run sums in registers, one addition per slice, 64 replicas - a sum of m terms is m - 1 binary additions,
    each off by at most u |partial sum| <= u A: (m - 1) u A to first order; the fixed-point sums of the record routes add
    exactly, so they only use less of it.  The slices of a sliced call are additions of that tree - a slice that holds
    nothing of an element adds nothing - so they are inside m - 1 and do not count again.  c counts the roundings inside
    one contribution, each at most u |w d| and so u A over the element; together with m - 1 the term has one to spare.
      atomic: 1.  k_scatter forms ((wx wy) wz) d and k_scatter_runs ((gx gy) gz) d: "the same multiplication order as the
              forward", which is the order of the oracle's w - the weight is the oracle's to the bit, the product with d
              is the one rounding (the oracle's own backward is this route with a sequential sum).
      pair:   6.  The record carries (a, b) = (wy wz) (d0, d1) and fx; the reduce forms (1 - fx) a and fx a: wy wz (1),
              times d (1), times the x share (1), against the oracle's (sx wy) wz (2 roundings of its own: the two
              differ by association), and the final float(double) of the fixed-point sum (1: the conversions of the
              slices round disjoint partial sums, together at most u A).  binary16 planes: wy wz (1), ws dx (1), gx a (1)
              in the reduce, the oracle's 2, the conversion: 6 again (1 - fx_q is exact: 23-bit fixed point).
      single: 2.  wk d with the forward's weight (1), the final conversion (1).
      coarse: 3.  wk d with the forward's weight (1); the register sums across lanes and stencil points are additions
              (inside m - 1); the gather table's sums leave as binary32 records (1: disjoint partial sums again), the
              reduce's final conversion (1).
      + 1 where the extra pair is summed first: |fl(a + b) - (a + b)| <= u (|a| + |b|), and A holds |w a| + |w b|.
    REDUCE TERM, record routes: k_bin_reduce scales a level by 2^k, k = 38 - e with Lmax < 2^e the level's largest emitted
    value, and rounds every record value to an integer: at most 2^-k / 2 = 2^(e - 39) <= Lmax 2^-38 per value, at most m
    values per element (fewer where the emit merged): m Lmax 2^-38.  Lmax: pair and single records report |d| (the pair
    after the binary32 sum with the extra pair: twice the largest |d|); coarse records hold a tile's sum for the element,
    at most the level's largest A (or a lone contribution the gather table had no slot for, at most the largest |d|),
    rounded to binary32 after at most mmax additions: (1 + (mmax + 4) u).
    GATHER TERM, coarse: the wave's gather table is 64-bit fixed point at 2^k2, k2 = 40 - ex, tmax < 2^ex the TILE's
    largest gradient (k_bin_emit): 2^(ex - 41) <= tmax 2^-40 per value added, at most m of them, tmax at most the level's
    largest |d| (twice that with an extra pair).
    REC16 TERM, "pair" with binary16 planes: w = wy wz and fx travel as 23-bit fixed point, |error| <= 2^-24 each
    (hashgrid.hip, Row12): |s_q w_q - s w| <= 2^-24 (w + s) + 2^-48 <= 2^-23 (1 + 2^-25) for the x share s and the weight w,
    times |d|: 2^-23 (1 + 2^-25) B.
    An element with m == 0 has bound 0: it must be exactly 0.0."""
    cfg = mdl.cfg
    out = {t: np.zeros(cfg.n_params) for t in TERMS}
    cs = []
    for l in range(cfg.n_levels):
        r, sl = routes[l], mdl.level_slice(l)
        m, A = mdl.m[sl].astype(np.float64), mdl.A[sl]
        summed = bool(extra_summed and mdl.has_extra and r != "atomic" and not (r == "pair" and half))
        c = ROUTE_C[r] + (1 if summed else 0)
        cs.append(c)
        out["binary32"][sl] = (m + c) * U * A
        dmax = mdl.dmax[l] * (2.0 if summed else 1.0)
        if r in RECORD_ROUTES:
            lmax = dmax if r != "coarse" else max(mdl.Amax[l], dmax) * (1.0 + (mdl.mmax[l] + 4) * U)
            out["reduce"][sl] = m * lmax * 2.0 ** -38
        if r == "coarse":
            out["gather"][sl] = m * dmax * 2.0 ** -40
        if r == "pair" and half:
            out["rec16"][sl] = 2.0 ** -23 * (1.0 + 2.0 ** -25) * mdl.B[sl]
    out["total"] = sum(out[t] for t in TERMS)
    out["total"][mdl.m == 0] = 0.0
    out["c"] = cs
    out["routes"] = list(routes)
    return out


def check_entries(g, mdl, bound):
    """Every table element of `g` against the model under `bound` (entry_bound's dict).  Returns (report, failures):
    report[l] = the level's route, c, worst err / bound, the element it occurred on (index into the table's floats), the
    term that dominated the bound there, how many elements miss the bound and how many must-be-zero elements are not zero;
    failures = the report rows of the levels with a miss."""
    g = np.asarray(g, np.float64)
    assert g.shape == mdl.ref.shape
    err, tot = np.abs(g - mdl.ref), bound["total"]
    report, failures = [], []
    for l in range(mdl.cfg.n_levels):
        sl = mdl.level_slice(l)
        e, b = err[sl], tot[sl]
        live = b > 0
        ratio = np.zeros(e.shape)
        with np.errstate(invalid="ignore", over="ignore"):
            ratio[live] = e[live] / b[live]
        ratio[live & ~np.isfinite(g[sl])] = np.inf                     # a NaN or inf is a miss, never `not greater than 1`
        nonzero = int(np.count_nonzero(g[sl][~live]))                  # bound 0: exactly 0.0 (-0.0 compares equal; NaN is not)
        misses = int(np.count_nonzero(~(ratio <= 1.0))) + nonzero
        i = int(np.argmax(ratio)) if ratio.size else 0
        at = sl.start + i
        row = {"level": l, "route": bound["routes"][l], "c": int(bound["c"][l]), "worst_ratio": float(ratio[i]) if ratio.size else 0.0,
               "element": at, "m": int(mdl.m[at]), "dominant_term": max(TERMS, key=lambda t: bound[t][at]),
               "misses": misses, "nonzero_where_zero_is_owed": nonzero}
        report.append(row)
        if misses:
            failures.append(row)
    return report, failures


def assert_entries(g, mdl, bound, what=""):
    report, failures = check_entries(g, mdl, bound)
    for row in report:
        print(what, row)
    assert not failures, f"{what}: per-entry bound missed on {len(failures)} level(s): {failures}"
    return report


def old_tolerance_misses(g, ref, rel=2e-5, abs_=1e-6):
    """What the global-maximum tolerance of the older tests flags, per element (kept to document the gap)."""
    return np.abs(np.asarray(g, np.float64) - ref) > rel * np.abs(ref).max() + abs_
