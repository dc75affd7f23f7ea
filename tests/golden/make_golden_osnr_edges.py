"""Writes tests/golden/osnr_edges.npz: admission checks at the edges of the GN-model GSNR kernel (csrc/orlg_osnr.hip) with
their 50-digit results.

    python tests/golden/make_golden_osnr_edges.py

Needs numpy and mpmath only -- neither the reference nor a GPU.  The file holds the flat arrays of `orlg_osnr_batch`
(include/orlg.h), `gsnr_db_mp` (oracle.gn_osnr_mp at 50 digits, rounded once to float64) and, per check, the index of its
case family in `family_names`.  tests/test_osnr.py asserts with a classifier of its own that the kernel paths and the
positions of the service's own list entry listed there are all present; `osnr_grid.npz` has none of the direct path and no
link of more than 64 spans.

What the families aim at (one wavefront per check, lanes over a link's list; see the kernel):
  direct_att   spans of one link differ in attenuation -> direct path; own entry absent / head / middle / tail / only
  direct_len   one attenuation, 513 and 700 entries -> direct path; 512 entries -> still the fast path
  fast_bounds  list lengths at the lane (64) and 8 x 64 boundaries, own entry at 0, 63, 64, n - 2, n - 1
  span_chunks  64, 65, 128, 129, 130 spans on both paths, own entry at the head: the stale phi comes from the span before,
               in the fast path's second chunk of 64 spans from the carry handed across the chunk boundary
  carry_links  an own-entry-at-head link after a fast link, a direct link, an empty list, a list of the own entry only, or
               as the first link of its check
  degenerate   no links, a link without spans (+inf dB), spans with an empty list
  se_bw_sides  all six spectral efficiencies, all three bandwidths, interferers below / above / around the service
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))

FAMILIES = ("direct_att", "direct_len", "fast_bounds", "span_chunks", "carry_links", "degenerate", "se_bw_sides")
GRID_HZ = 184.5e12 + 12.5e9 * np.arange(1072)     # L, C and S band in 12.5 GHz steps
BANDWIDTHS = (37.5e9, 50e9, 75e9)
DB_KM = 1 / (2 * 10 * np.log10(np.exp(1)) * 1e3)  # dB/km -> 1/m (the convention of gn_gate_parameters)


class Builder:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.check_link_off, self.link_span_off, self.link_svc_off = [0], [0], [0]
        self.check = []      # (bandwidth, center frequency, launch power)
        self.span = []       # (length km, attenuation, noise figure)
        self.svc = []        # (bandwidth, center frequency, se, is_self)
        self.family = []

    # values on coarse grids: few distinct doubles, so the file stays small
    def att(self):
        return float(self.rng.integers(36, 51)) * 0.005 * DB_KM

    def spans(self, n, uniform=True):
        a0 = self.att()
        out = []
        for j in range(n):
            a = a0
            while not uniform and j and a == out[j - 1][1]:      # neighbours differ, so no two-span link is uniform by chance
                a = self.att()
            out.append((float(self.rng.integers(80, 161)) * 0.5, a, float(10 ** (self.rng.integers(45, 66) / 100.0))))
        return out

    def services(self, n, own_at, fc, bw, side="both"):
        """n list entries, the check's own at index own_at (None: absent); nobody else sits on fc."""
        cand = GRID_HZ[GRID_HZ != fc]
        if side == "below":
            cand = cand[cand < fc]
        elif side == "above":
            cand = cand[cand > fc]
        others = n - (own_at is not None)
        f = self.rng.choice(cand, size=others, replace=False)
        out = [(float(self.rng.choice(BANDWIDTHS)), float(x), 1 + (i + int(self.rng.integers(0, 6))) % 6, 0) for i, x in enumerate(f)]
        if side != "both":          # every spectral efficiency, in turn
            out = [(b, x, 1 + i % 6, 0) for i, (b, x, _, _) in enumerate(out)]
        if own_at is not None:
            out.insert(own_at, (bw, fc, 1, 1))
        return out

    def add(self, family, links, bw=None, fc=None, side="both"):
        """links: (spans, n entries, index of the own entry or None), or a callable (fc, bw) -> (spans, list)"""
        bw = float(self.rng.choice(BANDWIDTHS)) if bw is None else bw
        fc = float(GRID_HZ[self.rng.integers(100, 972)]) if fc is None else fc
        pw = float(1e-3 * 10 ** (self.rng.integers(-6, 3) * 0.5 / 10))
        for spans, n, own_at in links:
            self.span += spans
            self.svc += self.services(n, own_at, fc, bw, side)
            self.link_span_off.append(len(self.span))
            self.link_svc_off.append(len(self.svc))
        self.check.append((bw, fc, pw))
        self.check_link_off.append(len(self.link_span_off) - 1)
        self.family.append(FAMILIES.index(family))

    def arrays(self):
        c, s, v = np.array(self.check).reshape(-1, 3), np.array(self.span).reshape(-1, 3), np.array(self.svc).reshape(-1, 4)
        return dict(check_link_off=np.array(self.check_link_off, np.int32), link_span_off=np.array(self.link_span_off, np.int32),
                    link_svc_off=np.array(self.link_svc_off, np.int32), bandwidth=c[:, 0].copy(), center_frequency=c[:, 1].copy(),
                    launch_power=c[:, 2].copy(), span_length_km=s[:, 0].copy(), span_attenuation=s[:, 1].copy(),
                    span_noise_figure=s[:, 2].copy(), svc_bandwidth=v[:, 0].copy(), svc_center_frequency=v[:, 1].copy(),
                    svc_se=v[:, 2].astype(np.int32), svc_is_self=v[:, 3].astype(np.uint8))


def own_positions(n):
    return {"absent": None, "head": 0, "middle": n // 2, "tail": n - 1}


def build(seed=20261):
    b = Builder(seed)
    rng = b.rng

    # --- direct path by attenuation: three links of one position class per check, short lists and lists of several lane rounds
    for lo, hi in ((4, 40), (66, 140)):
        for cls in ("absent", "head", "middle", "tail", "only"):
            links = []
            for _ in range(3):
                n = 1 if cls == "only" else int(rng.integers(lo, hi))
                links.append((b.spans(int(rng.integers(2, 6)), uniform=False), n, 0 if cls == "only" else own_positions(n)[cls]))
            b.add("direct_att", links)

    # --- direct path by length; 512 entries still take the fast path
    for n, classes in ((513, ("absent", "head", "middle", "tail")), (700, ("absent", "head", "middle")), (512, ("absent", "head", "tail"))):
        for cls in classes:
            b.add("direct_len", [(b.spans(2), n, own_positions(n)[cls])])

    # --- fast path: lane and 8 x 64 boundaries of the list length, own entry next to them
    for n in (1, 63, 64, 65, 128, 129, 511, 512):
        for own_at in sorted({p for p in (0, 63, 64, n - 1, n - 2) if 0 <= p < n}):
            b.add("fast_bounds", [(b.spans(3), n, own_at)])
        if n in (64, 65):
            b.add("fast_bounds", [(b.spans(3), n, None)])

    # --- chunks of 64 spans on both paths: a short link first, so that the carry into the long link is not 0
    for ns in (64, 65, 128, 129, 130):
        for uniform in (True, False):
            n = int(rng.integers(5, 12))
            b.add("span_chunks", [(b.spans(2), 6, None), (b.spans(ns, uniform=uniform), n, 0)])
    b.add("span_chunks", [(b.spans(130), 7, 6)])                                       # own entry at the tail, across chunks
    b.add("span_chunks", [(b.spans(2), 6, 5), (b.spans(130), 1, 0), (b.spans(2), 5, 0)])  # a list of the own entry only keeps the carry across chunks

    # --- the carry across links
    def short(uniform, own=None, n=None):
        n = int(rng.integers(3, 20)) if n is None else n
        return (b.spans(int(rng.integers(2, 5)), uniform=uniform), n, {"tail": n - 1, "middle": n // 2, "head": 0, None: None}[own])

    def before(kind):
        return {"first": [], "fast": [short(True, "tail")], "direct": [short(False, "middle")],
                "fast_empty": [short(True), short(True, n=0)], "direct_empty": [short(False, "tail"), short(False, n=0)],
                "fast_own_only": [short(True, "middle"), short(True, "head", n=1)],
                "direct_own_only": [short(False), short(False, "head", n=1)],
                "fast_own_only_direct": [short(True, "tail"), short(False, "head", n=1)]}[kind]

    for kind in ("first", "fast", "direct", "fast_empty", "direct_empty", "fast_own_only", "direct_own_only", "fast_own_only_direct"):
        for uniform in (True, False):
            b.add("carry_links", before(kind) + [short(uniform, "head")])
    b.add("carry_links", [short(False), short(True, "head"), short(False, "head"), short(True, "head", n=1), short(True, n=0),
                          short(False, "head", n=1), short(True, "head"), short(False, "head")])

    # --- degenerate
    b.add("degenerate", [])
    b.add("degenerate", [([], 5, None)])
    b.add("degenerate", [([], 0, None)])
    b.add("degenerate", [(b.spans(3), 0, None)])
    b.add("degenerate", [(b.spans(3, uniform=False), 0, None)])
    b.add("degenerate", [short(True), ([], 4, 0), short(True, "head")])    # a link without spans leaves the carry alone
    b.add("degenerate", [short(False), ([], 4, None), short(False, "head")])

    # --- all six spectral efficiencies, all three bandwidths, interferers on either side
    for bw in BANDWIDTHS:
        for side in ("below", "above", "both"):
            b.add("se_bw_sides", [(b.spans(3), 18, 7), (b.spans(3, uniform=False), 12, None)], bw=bw, side=side)
    return b.arrays(), np.array(b.family, np.int32)


def main():
    import oracle as orc
    arrays, family = build()
    mp_db = orc.gn_osnr_mp(arrays)
    path = os.path.join(HERE, "osnr_edges.npz")
    np.savez_compressed(path, **arrays, gsnr_db_mp=mp_db, family=family, family_names=np.array(FAMILIES))
    fin = np.isfinite(mp_db)
    print("osnr edges:", len(family), "checks,", len(arrays["link_span_off"]) - 1, "links,", len(arrays["span_length_km"]), "spans,",
          len(arrays["svc_bandwidth"]), "list entries;", os.path.getsize(path), "bytes; GSNR", mp_db[fin].min(), "..", mp_db[fin].max(),
          "dB,", int((~fin).sum()), "infinite")
    got = orc.gn_osnr(arrays)
    print("oracle vs 50 digits, worst relative:", np.max(np.abs(got[fin] - mp_db[fin]) / np.abs(mp_db[fin])),
          "; infinities equal:", bool(np.array_equal(got[~fin], mp_db[~fin])))


if __name__ == "__main__":
    main()
