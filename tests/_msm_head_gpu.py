"""GPU half of tests/test_gpu_msm_head.py, a process of its own with VIMZ_HIP_LIBRARY=testing (`python -m tests._msm_head_gpu GROUP OUT.json`): every case of one
group of tests/_msm_head_ref.py through the stage hooks of include/vimz_hip_testing.h (vimz_test_msm_sort, _accum, _small, _fixed, _ones, vimz_test_bases_tables), each
result held against the integer reference HERE — counters, offsets and sort entries word for word (a bucket's slice as a multiset), points as integers mod p and
inside the bounds of ec.hpp, the identity as ZZ = 0.  Writes {"ran": cases run, "failed": [[case, what]], "seconds": wall time of the cases} and prints the count.
Test infrastructure."""
import ctypes as C
import json
import sys
import time
import traceback

import numpy as np

from tests import _msm_head_ref as H
from tests import _msm_tail_ref as T
from tests._msm_tail_gpu import point_is

U32 = np.uint32


class Hooks:
    def __init__(self, ctx):
        from vimz_amd import hip
        self.ctx, self.lib, self.p = ctx, ctx.lib, hip._ptr
        vp, sz, i, u = C.c_void_p, C.c_size_t, C.c_int, C.c_uint32
        self.lib.vimz_test_msm_sort.argtypes = [vp, i, vp, sz, i, i, i, i, i, i, u, i, u, u, u, i, vp, vp, vp, vp, vp, sz]
        self.lib.vimz_test_msm_accum.argtypes = [vp, vp, vp, sz, vp, vp, vp, sz, u, sz, vp, sz]
        self.lib.vimz_test_msm_small.argtypes = [vp, vp, i, sz, vp, sz, i, i, u, u, i, i, vp]
        self.lib.vimz_test_msm_fixed.argtypes = [vp, vp, sz, vp, sz, i, i, i, vp]
        self.lib.vimz_test_msm_ones.argtypes = [vp, vp, vp, sz, sz, sz, i, i, vp]
        self.lib.vimz_test_bases_tables.argtypes = [vp, vp, i, i, vp, sz, vp]
        self.check = True
        self.keys = {}

    def _rc(self, rc):
        if self.check:
            self.ctx._chk(rc)
        return rc

    def key(self, c, ks, tables=0):
        """a key of the points k·G, uploaded once per (curve, ks, tables); tables: vimz_bases_precompute(tables)"""
        ident = (c, tuple(ks) if len(ks) < 64 else (len(ks), hash(tuple(ks))), tables)
        if ident not in self.keys:
            if sum(b.n for b in self.keys.values()) > 60000:      # (the tables of multiples are 151 KB a point: keep few keys resident)
                self.free_keys()
            b = self.ctx.bases_upload(c, H.key_points(c, ks))
            if tables:
                b.precompute(tables)
            self.keys[ident] = b
        return self.keys[ident]

    def free_keys(self):
        for b in self.keys.values():
            b.free()
        self.keys = {}

    def sort(self, case, words, calls=2, sorted_len=None, **over):
        a = {**case, **over}
        K, nbw, nb, _, pstride = H.sort_shape(a)
        K, nb = over.get("K", K), over.get("nb", nb)
        sc = H.words_u64(words)
        sorted_len = K * len(words) + 7 if sorted_len is None else sorted_len
        o = {"counts": np.full((calls, nb), 7, U32), "bucket_off": np.full((calls, nb + 1), 7, U32), "sub_off": np.full((calls, nb + 1), 7, U32),
             "totals": np.full((calls, 4), 7, U32), "sorted": np.full((calls, sorted_len), 7, U32)}
        self.rc = self._rc(self.lib.vimz_test_msm_sort(self.ctx.h, a["field"], self.p(sc), len(words), a["form"], a["skip_ones"], a["sgn"], a["c"], K, a["shared"], pstride, a["lds"],
                                                       a["sort_blocks"], a["sub"], H.SORT_HEAVY_MIN, calls, self.p(o["counts"]), self.p(o["bucket_off"]), self.p(o["sub_off"]),
                                                       self.p(o["totals"]), self.p(o["sorted"]), sorted_len))
        return o

    def accum(self, bases, srt, boff, soff, totals, sub, partial):
        srt, boff, soff, totals = (np.ascontiguousarray(a, dtype=U32) for a in (srt, boff, soff, totals))
        partial = np.array(partial, dtype=U32, order="C")
        rows, n_slots, _ = partial.shape
        self.rc = self._rc(self.lib.vimz_test_msm_accum(self.ctx.h, bases.h, self.p(srt), srt.shape[1], self.p(boff), self.p(soff), self.p(totals), boff.shape[1] - 1, sub, rows,
                                                        self.p(partial), n_slots))
        return partial

    def small(self, bases, c, tables, offset, words, form, sgn, Q, chunk, tail, calls):
        sc = H.words_u64(words)
        out = np.full((calls, H.windows(H.FIELD_P[H.SCALAR_FIELD[c]], H.SMALL_C), T.SLOT_WORDS), 7, dtype=U32)
        self.rc = self._rc(self.lib.vimz_test_msm_small(self.ctx.h, bases.h, int(tables), offset, self.p(sc), len(words), form, sgn, Q, chunk, tail, calls, self.p(out)))
        return out

    def fixed(self, bases, c, offset, words, form, sgn, calls):
        sc = H.words_u64(words)
        out = np.full((calls, H.windows(H.FIELD_P[H.SCALAR_FIELD[c]], H.SMALL_C), T.SLOT_WORDS), 7, dtype=U32)
        self.rc = self._rc(self.lib.vimz_test_msm_fixed(self.ctx.h, bases.h, offset, self.p(sc), len(words), form, sgn, calls, self.p(out)))
        return out

    def ones(self, bases, rows_words, form, kind):
        rows, n = len(rows_words), len(rows_words[0])
        sc = np.concatenate([H.words_u64(w) for w in rows_words])
        out = np.full((rows, T.SLOT_WORDS), 7, dtype=U32)
        self.rc = self._rc(self.lib.vimz_test_msm_ones(self.ctx.h, bases.h, self.p(sc), n, n, rows, form, kind, self.p(out)))
        return out

    def tables(self, bases, tc, which, wim):
        wim = np.ascontiguousarray(wim, dtype=U32).reshape(-1, 3)
        out = np.full((len(wim), 8), 7, dtype=np.uint64)
        self.rc = self._rc(self.lib.vimz_test_bases_tables(self.ctx.h, bases.h, tc, which, self.p(wim), len(wim), self.p(out)))
        return out


def xy_of(row):
    return tuple(int(row[4 * k]) | int(row[4 * k + 1]) << 64 | int(row[4 * k + 2]) << 128 | int(row[4 * k + 3]) << 192 for k in (0, 1))


# ---- groups -------------------------------------------------------------------------------------------------------------------------------------
def run_sort(h, name):
    case = H.sort_cases()[name]
    words = H.sort_words(case)
    K, nbw, nb, bstride, pstride = H.sort_shape(case)
    o = h.sort(case, words)
    counts, boff, soff, totals, ent = H.sort_ref(words, H.FIELD_P[case["field"]], case["form"], case["skip_ones"], case["sgn"], case["c"], K, bstride, pstride, nb, case["sub"])
    bad = []
    if ent:
        ea = np.array(ent, dtype=np.uint64)
        want = ea[np.lexsort((ea[:, 1], ea[:, 0])), 1]
    else:
        want = np.zeros(0, dtype=np.uint64)
    bucket_of = np.repeat(np.arange(nb), counts.astype(np.int64))
    for call in range(o["counts"].shape[0]):
        what = f"call {call}"
        for nm, w in (("counts", counts), ("bucket_off", boff), ("sub_off", soff)):
            if not np.array_equal(o[nm][call].astype(np.uint64), w):
                bad.append(f"{what}: {nm} differs")
        if o["totals"][call].tolist() != totals:
            bad.append(f"{what}: totals = {o['totals'][call].tolist()}, expected {totals}")
        got = o["sorted"][call]
        if not (got[len(want):] == H.UNWRITTEN).all():
            bad.append(f"{what}: a word of `sorted` past the {len(want)} entries was written")
        head = got[:len(want)].astype(np.uint64)
        if len(want) and (head == H.UNWRITTEN).any():
            bad.append(f"{what}: {int((head == H.UNWRITTEN).sum())} positions below totals[1] were never written")
        if not bad and not np.array_equal(head[np.lexsort((head, bucket_of))], want):
            bad.append(f"{what}: a bucket's slice of `sorted` is not the model's multiset")
    return bad


def run_accum(h, case):
    c, sub, total, rows = case
    bases = h.key(c, H.ACCUM_KEY)
    srt, boff, soff, totals, layouts = H.accum_arrays(sub, total, rows)
    n_slots = total + 3
    before = np.stack([T.garbage(n_slots)] * rows)
    out = h.accum(bases, srt, boff, soff, totals, sub, before)
    bad = []
    for r in range(rows):
        want = H.accum_ref(layouts[r], sub)
        assert len(want) == total
        for s, k in enumerate(want):
            e = point_is(c, out[r, s], k, f"row {r} slot {s}")
            if e:
                bad.append(e)
        if not np.array_equal(out[r, total:], before[r, total:]):
            bad.append(f"row {r}: a slot at or past totals[0] = {total} was written")
    return bad


def check_sums(c, out, want, what):
    bad = []
    for call in range(out.shape[0]):
        for w, k in enumerate(want):
            e = point_is(c, out[call, w], k, f"{what} call {call} window {w}")
            if e:
                bad.append(e)
    return bad


def run_small(h, name):
    case = H.small_cases()[name]
    c = case["curve"]
    words, ks = H.fused_inputs(case)
    n = len(words)
    Q, chunk = (case["Q"], case["chunk"]) if case["n"] is not None else (1, n)
    tables, offset = int(case["tables"]), case["offset"]
    bases = h.key(c, H.key_ks(offset + 3)[:offset] + ks + ([17] if tables else []), 7 if tables else 0)      # (with tables the row is longer than offset + n)
    out = h.small(bases, c, tables, offset, words, case["form"], case["sgn"], Q, chunk, case["tail"], case["calls"])
    want = H.window_sums_ref(c, words, ks, case["form"], case["sgn"], tables)
    assert H.fold_window_sums(c, want, tables) == H.msm_scalar(c, words, ks, case["form"])
    return check_sums(c, out, want, "k_msm_small")


def run_fixed(h, name):
    case = H.fixed_cases()[name]
    c, offset = case["curve"], case["offset"]
    words, ks = H.fused_inputs(case)
    bases = h.key(c, H.key_ks(offset + 3)[:offset] + ks + [17], 7)
    out = h.fixed(bases, c, offset, words, case["form"], case["sgn"], case["calls"])
    want = H.window_sums_ref(c, words, ks, case["form"], case["sgn"], 1)
    return check_sums(c, out, want, "k_msm_fixed")


def run_tables(h, case):
    c, tc, n = case
    bases = h.key(c, H.table_key(n), tc)
    ent = H.table_entries(c, tc, n)
    bad = []
    for which in (0, 1):
        sel = [e for e in ent if e[0] == which]
        if not sel:
            continue
        out = h.tables(bases, tc, which, [[w, i, m] for _, w, i, m, _ in sel])
        for (_, w, i, m, k), row in zip(sel, out):
            if xy_of(row) != (T.mul(c, k) if k else (0, 0)):
                bad.append(f"{'multiples' if which else 'window table'} entry (w = {w}, i = {i}, m = {m}) is not the point expected")
    return bad


def run_ones(h, name):
    case = H.ones_cases()[name]
    c, n = case["curve"], case["n"]
    p = H.FIELD_P[H.SCALAR_FIELD[c]]
    ks = H.key_ks(n)
    bases = h.key(c, ks)
    rows_words = [H.ones_words(c, n, case["form"], case["content"], r) for r in range(case["rows"])]
    out = h.ones(bases, rows_words, case["form"], case["kind"])
    bad = [point_is(c, out[r], H.ones_ref(rows_words[r], ks, p, case["form"]), f"row {r}") for r in range(case["rows"])]
    return [e for e in bad if e]


def run_invalid(h, rule):
    """one refusal (VIMZ_ERR_INVALID and a message) per validation rule, then a good call on the same context"""
    from vimz_amd import _lib
    c = 0
    sc = dict(field=0, form=0, sgn=1, skip_ones=0, c=7, shared=0, lds=1, n=65, sort_blocks=2, sub=8, kind="edges")
    words = H.sort_words(sc)
    srt, boff, soff, totals, _ = H.accum_arrays(8, 255, 1)
    part = np.stack([T.garbage(258)])
    key, key7 = h.key(c, H.ACCUM_KEY), h.key(c, H.key_ks(20), 7)
    w20 = H.scalar_words(0, 20, 7, 0)
    h.check = False
    try:
        if rule == "sort_lds_counters_past_144_KiB":
            h.sort({**sc, "c": 16, "shared": 0}, words)
        elif rule == "sort_c_outside_2_16":
            h.sort({**sc, "c": 17, "shared": 1}, words, K=16, nb=1 << 16)
        elif rule == "sort_blocks_outside_1_256":
            h.sort({**sc, "sort_blocks": 257}, words)
        elif rule == "sort_sorted_too_short":
            h.sort(sc, words, sorted_len=65 * 37 - 1)
        elif rule == "accum_offsets_not_monotone":
            b = boff.copy(); b[0, 9], b[0, 10] = b[0, 10], b[0, 9] + 1
            h.accum(key, srt, b, soff, totals, 8, part)
        elif rule == "accum_sub_off_inconsistent":
            s = soff.copy(); s[0, 8:] += 1
            h.accum(key, srt, boff, s, totals, 8, part)
        elif rule == "accum_index_outside_the_key":
            s = srt.copy(); s[0, 3] = len(H.ACCUM_KEY) | (1 << 31)
            h.accum(key, s, boff, soff, totals, 8, part)
        elif rule == "accum_rows_above_16":
            h.accum(key, np.repeat(srt, 17, 0), np.repeat(boff, 17, 0), np.repeat(soff, 17, 0), np.repeat(totals, 17, 0), 8, np.repeat(part, 17, 0))
        elif rule == "small_n_outside_the_chunks":
            h.small(key7, c, 0, 0, w20, 0, 1, 3, 10, 0, 1)
        elif rule == "small_chunk_above_1536":
            h.small(key7, c, 0, 0, w20, 0, 1, 1, 1537, 0, 1)
        elif rule == "small_Q_above_32":
            h.small(key7, c, 0, 0, w20, 0, 1, 33, 1, 0, 1)
        elif rule == "small_tables_missing":
            h.small(key, c, 1, 0, w20, 0, 1, 1, 20, 0, 1)
        elif rule == "fixed_tables_missing":
            h.fixed(key, c, 0, w20, 0, 1, 1)
        elif rule == "ones_rows_above_32":
            h.ones(key, [w20] * 33, 0, 2)
        elif rule == "ones_n_outside_the_key":
            h.ones(key7, [w20 + w20], 0, 1)
        elif rule == "tables_entry_outside":
            h.tables(key7, 7, 1, [[0, 20, 1]])
        else:
            raise ValueError(rule)
        rc, msg = h.rc, h.lib.vimz_last_error(h.ctx.h).decode()
    finally:
        h.check = True
    bad = [] if rc == _lib.ERR_INVALID and msg else [f"{rule}: returned {rc} with the message {msg!r}"]
    out = h.small(key7, c, 1, 0, w20, 0, 1, 1, 20, 0, 1)      # the context is still usable
    return bad + check_sums(c, out, H.window_sums_ref(c, w20, H.key_ks(20), 0, 1, 1), "the good call after the refusal")


RUN = {"sort": run_sort, "accum": run_accum, "small": run_small, "fixed": run_fixed, "tables": run_tables, "ones": run_ones, "invalid": run_invalid}


def main(group, out_path):
    from vimz_amd import _lib, hip
    assert _lib.SO_PATH == _lib.TESTING_SO_PATH, "start this script with VIMZ_HIP_LIBRARY=testing"
    ctx = hip.Context(0)
    res = {"ran": 0, "failed": [], "seconds": 0.0}
    t0 = time.time()
    h = None
    try:
        h = Hooks(ctx)
        for case in H.group_cases(group):
            try:
                bad = RUN[group](h, case)
            except Exception:      # noqa: BLE001 — a case that cannot run is a failed case; a HIP error ends the group (the context is gone)
                res["failed"].append([repr(case), traceback.format_exc()[-1500:]])
                break
            res["ran"] += 1
            if bad:
                res["failed"].append([repr(case), f"{len(bad)} wrong: " + "; ".join(bad[:4])])
    finally:
        res["seconds"] = round(time.time() - t0, 2)
        if h is not None and not res["failed"]:
            h.free_keys()
        ctx.close()
        with open(out_path, "w") as fp:
            json.dump(res, fp)
    print("msm head", group, "cases run:", res["ran"], "failed:", len(res["failed"]), "seconds:", res["seconds"])


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
