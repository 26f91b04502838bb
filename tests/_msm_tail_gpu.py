"""GPU half of tests/test_gpu_msm_tail.py, a process of its own with VIMZ_HIP_LIBRARY=testing (`python -m tests._msm_tail_gpu GROUP OUT.json`): every case of one
group of tests/_msm_tail_ref.py through the stage hooks of include/vimz_hip_testing.h (vimz_test_msm_scan, _combine, _reduce, _tree, vimz_test_quad_level), each
result held against the integer reference HERE — points as integers mod p and inside the bounds of ec.hpp, limbs word for word where the contract fixes them,
offsets and counters exactly.  Writes {"ran": cases run, "failed": [[case, what]]} and prints the count.  Test infrastructure."""
import ctypes as C
import json
import sys
import traceback

import numpy as np

from tests import _msm_tail_ref as T

U32 = np.uint32


class Hooks:
    def __init__(self, ctx):
        from vimz_amd import hip
        self.ctx, self.lib, self.p = ctx, ctx.lib, hip._ptr
        vp, sz, i, u = C.c_void_p, C.c_size_t, C.c_int, C.c_uint32
        self.lib.vimz_test_msm_scan.argtypes = [vp, vp, sz, sz, u, u, i, i, vp, vp, vp, vp, vp, vp]
        self.lib.vimz_test_msm_combine.argtypes = [vp, i, vp, sz, vp, sz, vp, sz, i, u, sz, i]
        self.lib.vimz_test_msm_reduce.argtypes = [vp, i, vp, sz, vp, vp, u, sz, i, sz, i, vp]
        self.lib.vimz_test_msm_tree.argtypes = [vp, i, vp, sz, sz, vp]
        self.lib.vimz_test_quad_level.argtypes = [vp, i, vp, sz, vp, sz, i, vp]
        self.check = True

    def _rc(self, rc):
        if self.check:
            self.ctx._chk(rc)
        return rc

    def quad(self, c, slots, levels, tree):
        slots = np.ascontiguousarray(slots, dtype=U32).reshape(-1, 256, T.SLOT_WORDS)
        out = np.full_like(slots, 7)
        lv = None if levels is None else np.ascontiguousarray(T.levels_words(levels))
        self.rc = self._rc(self.lib.vimz_test_quad_level(self.ctx.h, c, self.p(slots), len(slots), self.p(lv), 0 if lv is None else len(lv), int(tree), self.p(out)))
        return out

    def tree(self, c, points, m, count):
        points = np.ascontiguousarray(points, dtype=U32)
        out = np.full((max(count, 1), T.SLOT_WORDS), 7, dtype=U32)
        self.rc = self._rc(self.lib.vimz_test_msm_tree(self.ctx.h, c, self.p(points), m, count, self.p(out)))
        return out

    def scan(self, hist, sub, heavy_min, lds, calls=2):
        hist = np.ascontiguousarray(hist, dtype=U32)
        blocks, nb = hist.shape
        o = {"counts": np.full(nb, 7, U32), "bucket_off": np.full(nb + 1, 7, U32), "sub_off": np.full(nb + 1, 7, U32), "totals": np.full(4, 7, U32),
             "heavy": np.full(1 + T.HEAVY_CAP + T.HEAVY_GUARD, 7, U32), "prefixes": np.full_like(hist, 7)}
        self.rc = self._rc(self.lib.vimz_test_msm_scan(self.ctx.h, self.p(hist), blocks, nb, sub, heavy_min, lds, calls, self.p(o["counts"]), self.p(o["bucket_off"]),
                                                       self.p(o["sub_off"]), self.p(o["totals"]), self.p(o["heavy"]), self.p(o["prefixes"])))
        return o

    def combine(self, c, partial, sub_off, heavy, lane_bits, heavy_min, calls):
        partial = np.array(partial, dtype=U32, order="C")               # rows x n_slots x 40, folded in place
        sub_off, heavy = np.ascontiguousarray(sub_off, dtype=U32), np.ascontiguousarray(heavy, dtype=U32)
        rows, n_slots, _ = partial.shape
        self.rc = self._rc(self.lib.vimz_test_msm_combine(self.ctx.h, c, self.p(partial), n_slots, self.p(sub_off), sub_off.shape[1] - 1, self.p(heavy), heavy.shape[1] - 1,
                                                          lane_bits, heavy_min, rows, calls))
        return partial

    def reduce(self, c, partial, counts, sub_off, nbw, windows, mode, calls=1):
        partial, counts, sub_off = (np.ascontiguousarray(a, dtype=U32) for a in (partial, counts, sub_off))
        rows, n_slots, _ = partial.shape
        kout = {0: windows, 1: 2 * windows, 2: max(nbw, 1).bit_length() + 1}[mode]
        out = np.full((rows, kout, T.SLOT_WORDS), 7, dtype=U32)
        self.rc = self._rc(self.lib.vimz_test_msm_reduce(self.ctx.h, c, self.p(partial), n_slots, self.p(counts), self.p(sub_off), nbw, windows, mode, rows, calls, self.p(out)))
        return out


def point_is(c, slot, k, what):
    """None, or what is wrong with a slot that must hold k·G inside the bounds"""
    try:
        pt = T.unpack(c, slot)
    except T.BadSlot as e:
        return f"{what}: {e}"
    if pt != T.mul(c, k):          # (the identity only as ZZ = 0, limb for limb: unpack refuses a ZZ that is a non-zero multiple of p)
        return f"{what}: not the point expected (k = {k})"
    return None


def limbs_are(slot, want, what):
    return None if np.array_equal(np.asarray(slot, dtype=U32), np.asarray(want, dtype=U32)) else f"{what}: limbs differ from the contract's"


_packed = {}


def packed(c, key, make):
    """specs and their packed slots, made once per (curve, key)"""
    if (c, key) not in _packed:
        specs = make()
        _packed[(c, key)] = (specs, T.pack(c, specs))
    return _packed[(c, key)]


def check_levels(c, specs, slots, out, levels, what):
    ks, limbs = T.apply_levels(specs, slots, levels)
    bad = []
    for i in range(256):
        e = limbs_are(out[i], limbs[i], f"{what} slot {i}") if limbs[i] is not None else point_is(c, out[i], ks[i], f"{what} slot {i}")
        if e:
            bad.append(e)
    return bad


# ---- groups -------------------------------------------------------------------------------------------------------------------------------------
def run_quad_level(h, case):
    c, count, table = case
    if count == "planted":
        specs, level = T.planted_level(c)
        slots = T.pack(c, specs)
        out = h.quad(c, slots, [level], 0)[0]
        return check_levels(c, specs, slots, out, [level], "planted")
    sets = [packed(c, ("quad", kind), lambda kind=kind: T.content(c, kind, 256, "quad", kmax=600)) for kind in T.CONTENTS]
    level = T.quad_table(table, count)
    out = h.quad(c, np.stack([s[1] for s in sets]), [level], 0)
    bad = []
    for kind, (specs, slots), o in zip(T.CONTENTS, sets, out):
        bad += check_levels(c, specs, slots, o, [level], kind)
    return bad


def run_quad_tree(h, case):
    c, kind = case
    specs, slots = packed(c, ("quad", kind), lambda: T.content(c, kind, 256, "quad", kmax=600))
    out = h.quad(c, slots, None, 1)[0]
    bad = check_levels(c, specs, slots, out, T.TREE256_LEVELS, kind)
    e = point_is(c, out[0], T.scalar_sum(specs), "slot 0 is the sum")
    return bad + ([e] if e else [])


def run_tree256(h, case):
    c, m, kind = case
    specs, slots = packed(c, ("tree", m, kind), lambda: T.content(c, kind, m, "tree"))
    out = h.tree(c, slots, m, 0)
    e = point_is(c, out[0], T.scalar_sum(specs), "sum") or (limbs_are(out[0], slots[0], "one point comes back as it went in") if m == 1 else None)
    return [e] if e else []


def run_tree_rows(h, case):
    c, count, m = case
    sums = [packed(c, ("tree", m, T.CONTENTS[(i + 1) % 8]), lambda i=i: T.content(c, T.CONTENTS[(i + 1) % 8], m, "tree")) for i in range(count)]
    out = h.tree(c, np.concatenate([s[1] for s in sums]), m, count)
    bad = [point_is(c, out[i], T.scalar_sum(sums[i][0]), f"sum {i}") for i in range(count)]
    return [e for e in bad if e]


def check_scan(o, hist, sub, heavy_min, lds, what):
    counts, boff, soff, heavy, prefixes = T.scan_ref(hist, sub, heavy_min)
    bad = []
    for name, want in (("counts", counts), ("bucket_off", boff), ("sub_off", soff)):
        if not np.array_equal(o[name].astype(np.uint64), want):
            bad.append(f"{what}: {name} differs")
    if [int(x) for x in o["totals"]] != [int(soff[-1]), int(boff[-1]), 0, 0]:
        bad.append(f"{what}: totals = {o['totals'].tolist()}, expected [{soff[-1]}, {boff[-1]}, 0, 0] (sub-buckets, entries, tickets back at zero)")
    n = int(o["heavy"][0])
    kept = min(n, T.HEAVY_CAP)
    ids = o["heavy"][1:1 + kept].tolist()
    if n != len(heavy) or len(set(ids)) != kept or not set(ids) <= heavy:
        bad.append(f"{what}: heavy count {n} (expected {len(heavy)}) or ids that are not {kept} distinct heavy buckets")
    if not (o["heavy"][1 + kept:] == 0xffffffff).all():
        bad.append(f"{what}: a word past the heavy list's ids was written")
    if lds and not np.array_equal(o["prefixes"].astype(np.uint64), prefixes):
        bad.append(f"{what}: the per-block prefixes differ")
    return bad


def run_scan(h, case):
    if case[0] == "overflow":
        sub, hist = T.SCAN_OVERFLOW["sub"], T.scan_overflow_counts()[None, :]
    else:
        nb, kind, sub, blocks = case
        hist = T.split_over_blocks(T.scan_counts(nb, kind, sub), blocks)
    outs = {lds: h.scan(hist, sub, T.SCAN_HEAVY_MIN, lds) for lds in (1, 0)}
    bad = check_scan(outs[1], hist, sub, T.SCAN_HEAVY_MIN, 1, "k_prefix_scan") + check_scan(outs[0], hist, sub, T.SCAN_HEAVY_MIN, 0, "k_scan")
    for name in ("counts", "bucket_off", "sub_off"):
        if not np.array_equal(outs[0][name], outs[1][name]):
            bad.append(f"{name}: the two scans disagree")
    return bad


def run_combine(h, case):
    c, name = case
    lane_bits, rows, calls, kind = T.COMBINE_CASES[name]
    layout = [T.combine_sizes(name, r) for r in range(rows)]
    data = []
    for r in range(rows):
        seed, make = T.combine_specs(c, name, r)
        data.append(packed(c, ("combine", seed, r), lambda: [s for b in make() for s in b]))
    nb = len(layout[0][0])
    assert all(len(m) == nb for m, _, _ in layout)
    n_slots = max(sum(m) for m, _, _ in layout) + 3
    n_ids = max(len(ids) for _, ids, _ in layout)
    partial = np.stack([np.concatenate([slots, T.garbage(n_slots - len(slots))]) for _, slots in data])
    sub_off = np.array([np.concatenate([[0], np.cumsum(m)]) for m, _, _ in layout], dtype=U32)
    heavy = np.zeros((rows, 1 + n_ids), dtype=U32)
    for r, (_, ids, count) in enumerate(layout):
        heavy[r, 0], heavy[r, 1:1 + len(ids)] = count, ids
    out = h.combine(c, partial, sub_off, heavy, lane_bits, T.heavy_min_of(lane_bits), calls)
    bad = []
    for r, (m, _, _) in enumerate(layout):
        specs = data[r][0]
        for b, size in enumerate(m):
            s0 = int(sub_off[r, b])
            if size == 0:
                continue
            what = f"row {r} bucket {b} of {size} partials"
            e = limbs_are(out[r, s0], partial[r, s0], what) if size == 1 else point_is(c, out[r, s0], T.scalar_sum(specs[s0:s0 + size]), what)
            if e:
                bad.append(e)
        if not np.array_equal(out[r, sum(m):], partial[r, sum(m):]):
            bad.append(f"row {r}: a slot past the last bucket was written")
    return bad


def reduce_inputs(c, nbw, kinds, seed):
    """(partial rows x n_slots x 40, counts, sub_off, ks[r][w]: the buckets' scalars with the empty ones at zero)"""
    rows, W = len(kinds), len(kinds[0])
    parts, cnts, offs, ks = [], [], [], []
    for r in range(rows):
        specs, counts = [], []
        for w in range(W):
            s, n = T.window_specs(c, kinds[r][w], nbw, f"{seed}/{r}/{w}")
            specs += s
            counts += n
        soff, first = T.bucket_layout(counts)
        part = T.garbage(int(soff[-1]) + 1)
        live = [g for g, n in enumerate(counts) if n]
        if live:
            part[first[live]] = T.pack(c, [specs[g] for g in live])
        parts.append(part); cnts.append(counts); offs.append(soff)
        ks.append([[s[0] if n else 0 for s, n in zip(specs[w * nbw:(w + 1) * nbw], counts[w * nbw:(w + 1) * nbw])] for w in range(W)])
    return np.stack(parts), np.array(cnts, dtype=U32), np.stack(offs), ks


def run_reduce(h, case):
    c, nbw, W, rows, kinds = case
    partial, counts, sub_off, ks = reduce_inputs(c, nbw, kinds, "reduce")
    out = h.reduce(c, partial, counts, sub_off, nbw, W, 0)
    bad = [point_is(c, out[r, w], T.reduce_ref(ks[r][w], [1] * nbw)[0], f"row {r} window {w} ({kinds[r][w]})") for r in range(rows) for w in range(W)]
    return [e for e in bad if e]


def run_reduce_plain(h, case):
    c, V = case
    kinds = [[T.REDUCE_BUCKETS[(v + 4) % 8] for v in range(V)]]
    partial, counts, sub_off, ks = reduce_inputs(c, 1024, kinds, "plain")
    out = h.reduce(c, partial, counts, sub_off, 1024, V, 1)
    bad = []
    for v in range(V):
        weighted, plain = T.reduce_ref(ks[0][v], [1] * 1024)
        bad += [point_is(c, out[0, v], weighted, f"R_{v} ({kinds[0][v]})"), point_is(c, out[0, V + v], plain, f"S_{v} ({kinds[0][v]})")]
    return [e for e in bad if e]


PLANES_KINDS = ("full_distinct", "zero_counts_over_garbage", "alternating_q_minus_q", "only_top_bucket", "all_empty")


def run_reduce_planes(h, case):
    c, nbw = case
    bad = []
    for kind in PLANES_KINDS:
        partial, counts, sub_off, ks = reduce_inputs(c, nbw, [[kind]], "planes")
        out = h.reduce(c, partial, counts, sub_off, nbw, 1, 2, calls=2)
        want = T.planes_ref(ks[0][0], [1] * nbw)
        assert len(want) == out.shape[1]
        bad += [point_is(c, out[0, i], k, f"{kind}: sum {i} of {len(want)}") for i, k in enumerate(want)]
    return [e for e in bad if e]


def run_invalid(h, rule):
    """one refusal (VIMZ_ERR_INVALID and a message) per validation rule, then a good call on the same context"""
    from vimz_amd import _lib
    c = 0
    specs, slots = packed(c, ("quad", "generic"), lambda: T.content(c, "generic", 256, "quad", kmax=600))
    partial, counts, sub_off, _ = reduce_inputs(c, 16, [["full_distinct"]], "invalid")
    m = [2, 3, 40, 1]
    cp = np.stack([np.concatenate([T.pack(c, T.content(c, "generic", sum(m), "invalid")), T.garbage(3)])])
    coff, cheavy = np.array([np.concatenate([[0], np.cumsum(m)])], dtype=U32), np.array([[1, 2]], dtype=U32)
    h.check = False
    try:
        if rule == "offsets_not_monotone":
            off = sub_off.copy(); off[0, 3], off[0, 4] = off[0, 4], off[0, 3]
            h.reduce(c, partial, counts, off, 16, 1, 0)
        elif rule == "offsets_outside_the_array":
            h.combine(c, cp[:, :sum(m) - 1], coff, cheavy, 1, 32, 1)
        elif rule == "bucket_id_not_below_nb":
            h.combine(c, cp, coff, np.array([[1, len(m)]], dtype=U32), 1, 32, 1)
        elif rule == "index_not_below_256":
            h.quad(c, slots, [([0, 1], [5, 256])], 0)
        elif rule == "dst_twice_in_a_level":
            h.quad(c, slots, [([0, 9, 0], [5, 6, 7])], 0)
        elif rule == "nbw_not_a_power_of_two":
            h.reduce(c, partial, counts, sub_off, 24, 1, 0)
        elif rule == "nbw_above_32768":
            h.reduce(c, partial, counts, sub_off, 65536, 1, 0)
        elif rule == "rows_above_16":
            h.reduce(c, np.repeat(partial, 17, axis=0), np.repeat(counts, 17, axis=0), np.repeat(sub_off, 17, axis=0), 16, 1, 0)
        else:
            raise ValueError(rule)
        rc, msg = h.rc, h.lib.vimz_last_error(h.ctx.h).decode()
    finally:
        h.check = True
    bad = [] if rc == _lib.ERR_INVALID and msg else [f"{rule}: returned {rc} with the message {msg!r}"]
    level = T.quad_table("scattered", 17)
    out = h.quad(c, slots, [level], 0)[0]                   # the context is still usable
    ok = h.combine(c, cp, coff, cheavy, 1, 32, 1)
    e = point_is(c, ok[0, 5], T.scalar_sum(T.content(c, "generic", sum(m), "invalid")[5:45]), "the good combine after the refusal")
    return bad + check_levels(c, specs, slots, out, [level], "the good call after the refusal") + ([e] if e else [])


RUN = {"quad_level": run_quad_level, "quad_tree": run_quad_tree, "tree256": run_tree256, "tree_rows": run_tree_rows, "scan": run_scan, "combine": run_combine,
       "reduce": run_reduce, "reduce_plain": run_reduce_plain, "reduce_planes": run_reduce_planes, "invalid": run_invalid}


def main(group, out_path):
    from vimz_amd import _lib, hip
    assert _lib.SO_PATH == _lib.TESTING_SO_PATH, "start this script with VIMZ_HIP_LIBRARY=testing"
    ctx = hip.Context(0)
    res = {"ran": 0, "failed": []}
    try:
        h = Hooks(ctx)
        for case in T.group_cases(group):
            try:
                bad = RUN[group](h, case)
            except Exception:      # noqa: BLE001 — a case that cannot run is a failed case; a HIP error ends the group (the context is gone)
                res["failed"].append([repr(case), traceback.format_exc()[-1500:]])
                break
            res["ran"] += 1
            if bad:
                res["failed"].append([repr(case), f"{len(bad)} wrong: " + "; ".join(bad[:4])])
    finally:
        ctx.close()
        with open(out_path, "w") as fp:
            json.dump(res, fp)
    print("msm tail", group, "cases run:", res["ran"], "failed:", len(res["failed"]))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
