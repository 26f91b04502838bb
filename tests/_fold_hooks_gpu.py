"""Body of tests/test_gpu_fold_kernels.py::test_fold_kernels_behind_the_test_hooks, run as a process of its own with VIMZ_HIP_LIBRARY=testing: k_fold_cross,
k_fold5, k_fresh_cross_neg and the two counting kernels (vimz_test_fold_cross, vimz_test_fold5, vimz_test_fresh_cross_neg, vimz_test_count) against Python
integers (tests/_fold_ref.py), and the lookahead schedule of a fold driven through the hooks against the direct fold.  Test infrastructure.

Every vector is two elements longer than the kernel's n, outputs pre-filled, and compared over its whole length, in Montgomery form word for word (v·2^256 mod
p: a representative at or above p fails); every input is downloaded again after the call and compared too."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import _fold_ref as fr      # noqa: E402
from vimz_amd import _lib              # noqa: E402

FIELDS = (0, 1, 2, 3)
N_FOLD_CROSS = sum(len(fr.fold_cross_cases(f)) for f in FIELDS)
N_FOLD5 = len(FIELDS) * len(fr.fold5_cases())
N_FRESH_NEG = len(fr.FRESH_NEG_FIELDS) * len(fr.fresh_neg_cases())
N_COUNT = sum(len(fr.count_cases(_lib.MODULUS[f], f)) for f in FIELDS)
N_SCHEDULE = fr.SCHEDULE_ROWS
N_REFUSED = 12
PAD = 2
MONT = _lib.FORM_MONTGOMERY


def _u(x):
    return np.array([(int(x) >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)], dtype=np.uint64)


def _words(p, vals, total=None):
    """what the device holds: the Montgomery words of vals, then the fill up to `total` elements"""
    total = len(vals) + PAD if total is None else total
    return np.concatenate([fr.to_limbs(fr.mont(p, vals)), fr.to_limbs([fr.FILL] * (total - len(vals)))])


class Run:
    def __init__(self):
        from vimz_amd import hip
        assert _lib.SO_PATH == _lib.TESTING_SO_PATH, "start this script with VIMZ_HIP_LIBRARY=testing"
        self.hip = hip
        self.ctx = hip.Context(0)
        lib = self.lib = self.ctx.lib
        vp, sz, ci, cu = C.c_void_p, C.c_size_t, C.c_int, C.c_uint
        lib.vimz_test_fold_cross.argtypes = [vp, sz, vp, vp, vp, vp, vp, ci, vp, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, ci, vp, sz, cu]
        lib.vimz_test_fold5.argtypes = [vp, vp, vp, vp, vp, vp, vp, ci, cu]
        lib.vimz_test_fresh_cross_neg.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp, vp, cu]
        lib.vimz_test_count.argtypes = [vp, ci, sz, vp, vp, vp]
        lib.vimz_test_cross_term_masked.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp, vp, vp, ci, vp, vp, sz]

    def up(self, fid, words):
        return self.ctx.vec_from_host(fid, words, form=MONT)

    def check(self, vec, want, what):
        got = vec.download(form=MONT)
        if got.shape == want.shape and np.array_equal(got, want):
            return
        assert got.shape == want.shape, f"{what}: {got.shape} elements for {want.shape}"
        bad = np.nonzero((got != want).any(axis=1))[0]
        g, w = fr.from_limbs(got[bad[0]])[0], fr.from_limbs(want[bad[0]])[0]
        raise AssertionError(f"{what}: {len(bad)} of {len(want)} elements differ, first {int(bad[0])} (wave {int(bad[0]) // 64} lane {int(bad[0]) % 64}): got {g:#x} want {w:#x}")

    @staticmethod
    def h(v):
        return v.h if v is not None else None

    # ---- the hooks with the reference's arguments ----------------------------------------------------------------------------------------------------
    def fold_cross(self, n, AZ, BZ, CZ, E, Tin, fold_E, r, hasB, r_prev, negB, u1, az, bz, cz, out, azn, bzn, czn, u2, outm, nb, blocks):
        h, s = self.h, lambda x: self.hip._ptr(_u(x))
        return self.lib.vimz_test_fold_cross(self.ctx.h, n, h(AZ), h(BZ), h(CZ), h(E), h(Tin), fold_E, s(r), hasB, s(r_prev), h(negB), s(u1), h(az), h(bz), h(cz), h(out),
                                             h(azn), h(bzn), h(czn), s(u2), _lib.FORM_CANONICAL, h(outm), nb, blocks)

    def fold5(self, x1, off1, x2, off2, ns, r, blocks):
        P5, S5 = C.c_void_p * 5, C.c_size_t * 5
        raw = lambda vs: P5(*[v.h.value if v is not None else None for v in vs])
        return self.lib.vimz_test_fold5(self.ctx.h, raw(x1), S5(*off1), raw(x2), S5(*off2), S5(*ns), self.hip._ptr(_u(r)), _lib.FORM_CANONICAL, blocks)


# ---- k_fold_cross ---------------------------------------------------------------------------------------------------------------------------------------------

def run_fold_cross(R):
    ran = 0
    for fid in FIELDS:
        p = _lib.MODULUS[fid]
        cls = fr.scalar_classes(p, f"fc:{fid}")
        u2_random = fr.scalars(p, f"fc:{fid}:u2")[3]
        data = {}
        for layout, n, blocks, o in fr.fold_cross_cases(fid):
            if (layout, n) not in data:
                for d in data.values():          # (the cases come layout by layout, size by size)
                    for v in d["dev"].values():
                        v.free()
                data.clear()
                host = fr.fresh_operands(p, layout, n, f"fc:{fid}", fr.FRESH + ("negB",))
                host.update(fr.running_operands(p, n, f"fc:{fid}:{layout}"))
                host["Tin"] = fr.tin_vector(p, layout, n, f"fc:{fid}")
                words = {k: _words(p, v) for k, v in host.items()}
                data[layout, n] = {"host": host, "words": words, "dev": {k: R.up(fid, words[k]) for k in fr.FRESH + ("negB", "Tin")}}
            d = data[layout, n]
            host, words, dev = d["host"], d["words"], d["dev"]
            fold_E, hasB = o["fold_E"], o["hasB"]
            r, r_prev, u1, u2 = cls[o["r"]], cls[o["r_prev"]], cls[o["u1"]], (1 if o["u2"] == 0 else u2_random)
            want_outm = o["out"] != "none" and o["nb"] is not None
            nb = fr.resolve_nb(o["nb"], n) if want_outm else 0
            what = f"k_fold_cross field {fid} {layout} n {n} blocks {blocks} {o}"
            run = {k: R.up(fid, words[k]) for k in ("AZ", "BZ", "CZ", "E")}
            fill = fr.to_limbs([fr.FILL] * (n + PAD))
            # Tin: the shared vector; a copy of its own when out overwrites it; NULL where the kernel must not read it (every other such case)
            if o["out"] == "alias":
                tin = out = R.up(fid, words["Tin"])
            else:
                tin = None if not fold_E and ran % 2 else dev["Tin"]
                out = R.up(fid, fill) if o["out"] == "separate" else None
            negB = None if not (fold_E and hasB) and ran % 2 else dev["negB"]
            outm = R.up(fid, fill) if want_outm else None
            nxt = [dev[k] if out is not None else None for k in ("azn", "bzn", "czn")]
            rc = R.fold_cross(n, run["AZ"], run["BZ"], run["CZ"], run["E"], tin, fold_E, r, hasB, r_prev, negB, u1, dev["az"], dev["bz"], dev["cz"], out, *nxt, u2, outm, nb, blocks)
            R.ctx._chk(rc)
            a, b, c, e, t, tm = fr.fold_cross(p, host["AZ"], host["BZ"], host["CZ"], host["E"], host["Tin"], fold_E, r, hasB, r_prev, host["negB"], u1, host["az"], host["bz"],
                                              host["cz"], out is not None, host["azn"], host["bzn"], host["czn"], u2, want_outm, nb)
            if fold_E:      # E stays as it was wherever the folded vector is zero (the reference says so; said here once more, on the input's own words)
                zero = [i for i, x in enumerate(fr.folded_vector(p, host["Tin"], hasB, r_prev, host["negB"])) if x == 0]
                assert all(e[i] == host["E"][i] for i in zero)
                got_E = run["E"].download(form=MONT)
                assert np.array_equal(got_E[zero], words["E"][zero]), f"{what}: E changed where the folded vector is zero"
            for k, v in (("AZ", a), ("BZ", b), ("CZ", c), ("E", e)):
                R.check(run[k], _words(p, v), f"{what}: {k}")
            if out is not None:
                R.check(out, _words(p, t), f"{what}: out")
            if outm is not None:
                R.check(outm, _words(p, tm), f"{what}: outm")
            for k, v in dev.items():            # the inputs, Tin among them unless out took its place (then the shared one was not passed at all)
                R.check(v, words[k], f"{what}: input {k} changed")
            for v in list(run.values()) + [x for x in (out, outm) if x is not None]:
                v.free()
            ran += 1
        for d in data.values():
            for v in d["dev"].values():
                v.free()
    return ran


# ---- k_fold5 --------------------------------------------------------------------------------------------------------------------------------------------------

def run_fold5(R):
    ran = 0
    for fid in FIELDS:
        p = _lib.MODULUS[fid]
        cls = fr.scalar_classes(p, f"f5:{fid}")
        made = {}
        for shape, layout, rc, blocks in fr.fold5_cases():
            lens, skip, off1, off2 = fr.FOLD5_SHAPES[shape]
            if (shape, layout) not in made:
                for m in made.values():
                    for v in m["x2"]:
                        v.free()
                made.clear()
                x2h = [fr.fresh_operands(p, layout, lens[v], f"f5:{fid}:{shape}:{v}", names=("x",))["x"] for v in range(5)]
                x1h = [fr.running_operands(p, lens[v], f"f5:{fid}:{shape}:{v}", names=("x",))["x"] for v in range(5)]
                # x2: the range behind off2 elements of fill; x1: the same behind off1 — the groups of FOLD5_SHARED as two ranges of ONE vector
                x2w = [np.concatenate([fr.to_limbs([fr.FILL] * off2[v]), _words(p, x2h[v])]) for v in range(5)]
                x1w = [np.concatenate([fr.to_limbs([fr.FILL] * off1[v]), _words(p, x1h[v])]) for v in range(5)]
                s0, s1 = fr.FOLD5_SHARED
                at = list(off1)
                at[s1] = len(x1w[s0]) + off1[s1]
                assert at[s1] % 64 and s0 != skip and s1 != skip
                x1w[s0] = np.concatenate([x1w[s0], x1w[s1]])
                made[shape, layout] = {"x2h": x2h, "x1h": x1h, "x2w": x2w, "x1w": x1w, "at": at, "x2": [R.up(fid, w) for w in x2w]}
            m = made[shape, layout]
            s0, s1 = fr.FOLD5_SHARED
            r = cls[rc]
            what = f"k_fold5 field {fid} shape {lens} x2 {layout} r class {rc} blocks {blocks}"
            x1 = [None if v in (skip, s1) else R.up(fid, m["x1w"][v]) for v in range(5)]
            x1[s1] = x1[s0]
            R.ctx._chk(R.fold5(x1, m["at"], m["x2"], off2, lens, r, blocks))
            want = fr.fold5(p, [(None if v == skip else m["x1h"][v], m["x2h"][v]) for v in range(5)], r)
            for v in range(5):
                if v in (skip, s1):
                    continue
                w = m["x1w"][v].copy()
                for q in ((s0, s1) if v == s0 else (v,)):
                    w[m["at"][q]:m["at"][q] + lens[q]] = fr.to_limbs(fr.mont(p, want[q]))
                R.check(x1[v], w, f"{what}: x1 of group {v}")
                x1[v].free()
            for v in range(5):
                R.check(m["x2"][v], m["x2w"][v], f"{what}: x2 of group {v} changed")
            ran += 1
        for m in made.values():
            for v in m["x2"]:
                v.free()
    return ran


# ---- k_fresh_cross_neg ------------------------------------------------------------------------------------------------------------------------------------------

def run_fresh_neg(R):
    ran = 0
    names = ("az0", "bz0", "cz0", "az1", "bz1", "cz1")
    for fid in fr.FRESH_NEG_FIELDS:
        p = _lib.MODULUS[fid]
        made = None
        for layout, n, blocks in fr.fresh_neg_cases():
            if made is None or made[0] != (layout, n):
                if made is not None:
                    for v in made[2]:
                        v.free()
                host = fr.fresh_operands(p, layout, n, f"fn:{fid}", names)
                words = [_words(p, host[k]) for k in names]
                made = ((layout, n), words, [R.up(fid, w) for w in words], _words(p, fr.fresh_cross_neg(p, *[host[k] for k in names])))
            _, words, dev, want = made
            out = R.up(fid, fr.to_limbs([fr.FILL] * (n + PAD)))
            R.ctx._chk(R.lib.vimz_test_fresh_cross_neg(R.ctx.h, n, *[v.h for v in dev], out.h, blocks))
            what = f"k_fresh_cross_neg field {fid} {layout} n {n} blocks {blocks}"
            R.check(out, want, f"{what}: out")
            out.free()
            for k, v, w in zip(names, dev, words):
                R.check(v, w, f"{what}: input {k} changed")
            ran += 1
        for v in made[2]:
            v.free()
    return ran


# ---- the counting kernels -----------------------------------------------------------------------------------------------------------------------------------------

def run_count(R):
    ran = 0
    for fid in FIELDS:
        for what, name, a, b, n, want in fr.count_cases(_lib.MODULUS[fid], fid):
            av = R.up(fid, fr.to_limbs(a))        # (raw words: the Montgomery form is copied as it lies)
            bv = R.up(fid, fr.to_limbs(b)) if b is not None else None
            got = []
            for _ in range(2):                    # twice on the same vectors: the hook starts from a zeroed counter
                cnt = C.c_uint64(12345)
                R.ctx._chk(R.lib.vimz_test_count(R.ctx.h, what, n, av.h, R.h(bv), C.byref(cnt)))
                got.append(cnt.value)
            assert got == [want, want], f"{('k_count_unreduced', 'k_count_diff')[what]} field {fid} {name}: counted {got}, want {want} both times"
            R.check(av, fr.to_limbs(a), f"count field {fid} {name}: a changed")
            av.free()
            if bv is not None:
                bv.free()
            ran += 1
    return ran


# ---- the lookahead schedule ---------------------------------------------------------------------------------------------------------------------------------------

def run_schedule(R):
    fid = 0
    p = _lib.MODULUS[fid]
    n = fr.SCHEDULE_N
    rinv = pow(fr.R, -1, p)
    rows = fr.satisfied_rows(p, n, fr.SCHEDULE_ROWS, "schedule")
    cls = fr.scalar_classes(p, "schedule")
    ch = [cls[3], cls[3] ^ 3, cls[4], cls[3] ^ 5, cls[1], cls[3] ^ 9]        # 128-bit challenges as the product's, a full-width one and 1
    up = lambda v: R.up(fid, _words(p, v)) if v is not None else None

    def down(vec, what):
        w = vec.download(form=MONT)
        vals = fr.from_limbs(w)
        assert all(x < p for x in vals[:n]) and np.array_equal(w[n:], fr.to_limbs([fr.FILL] * PAD)), f"schedule {what}: a word not below p, or the tail written"
        return [x * rinv % p for x in vals[:n]]

    def fold_cross_fn(p_, AZ, BZ, CZ, E, Tin, fold_E, r, hasB, r_prev, negB, u1, az, bz, cz, out, azn, bzn, czn, u2, outm, nb):
        d = [up(v) for v in (AZ, BZ, CZ, E, Tin, negB, az, bz, cz, azn, bzn, czn)]
        o = d[4] if out == "alias" else R.up(fid, fr.to_limbs([fr.FILL] * (n + PAD))) if out else None
        R.ctx._chk(R.fold_cross(n, d[0], d[1], d[2], d[3], d[4], fold_E, r, hasB, r_prev, d[5], u1, d[6], d[7], d[8], o, d[9], d[10], d[11], u2, None, 0, 0))
        res = [down(v, "fold_cross") for v in d[:4]] + [down(o, "out") if o is not None else None, None]
        if out != "alias":
            R.check(d[4], _words(p, Tin), "schedule: Tin changed")
        for v in d + ([o] if out == "separate" else []):
            if v is not None:
                v.free()
        return res

    def fresh_cross_neg_fn(p_, *six):
        d = [up(v) for v in six]
        o = R.up(fid, fr.to_limbs([fr.FILL] * (n + PAD)))
        R.ctx._chk(R.lib.vimz_test_fresh_cross_neg(R.ctx.h, n, *[v.h for v in d], o.h, 0))
        res = down(o, "negB")
        for v in d + [o]:
            v.free()
        return res

    def cross_term_fn(p_, AZ, BZ, CZ, u, az, bz, cz, u2):
        d = [up(v) for v in (AZ, BZ, CZ, az, bz, cz)]
        o = R.up(fid, fr.to_limbs([fr.FILL] * (n + PAD)))
        R.ctx._chk(R.lib.vimz_test_cross_term_masked(R.ctx.h, n, d[0].h, d[1].h, d[2].h, R.hip._ptr(_u(u)), d[3].h, d[4].h, d[5].h, R.hip._ptr(_u(u2)), _lib.FORM_CANONICAL, o.h, None, 0))
        res = down(o, "cross term")
        for v in d + [o]:
            v.free()
        return res

    states = fr.direct_chain(p, rows, ch)
    ran = 0
    for st, AZ, BZ, CZ, E, t, out in fr.run_schedule(p, rows, ch, fold_cross_fn, fresh_cross_neg_fn, cross_term_fn):
        want = states[st["i"]]
        for k, v in (("AZ", AZ), ("BZ", BZ), ("CZ", CZ), ("E", E)):
            bad = [i for i in range(n) if v[i] != want[k][i]]
            assert not bad, f"schedule step {st}: {k} differs from the direct fold on {len(bad)} elements, first {bad[0]}: got {v[bad[0]]:#x} want {want[k][bad[0]]:#x}"
        if t is not None:
            ref = fr.cross_term(p, want["AZ"], want["BZ"], want["CZ"], want["u"], *rows[t], 1)
            bad = [i for i in range(n) if out[i] != ref[i]]
            assert not bad, f"schedule step {st}: the cross term for row {t} differs on {len(bad)} elements, first {bad[0]}"
        ran += 1
    return ran


# ---- what the hooks refuse (nothing is launched) ------------------------------------------------------------------------------------------------------------------

def run_refused(R):
    n = 8
    v = [R.ctx.vec_alloc(0, n) for _ in range(14)]
    short, other = R.ctx.vec_alloc(0, n - 1), R.ctx.vec_alloc(1, n)
    AZ, BZ, CZ, E, Tin, negB, az, bz, cz, out, azn, bzn, czn, outm = v
    good = dict(n=n, AZ=AZ, BZ=BZ, CZ=CZ, E=E, Tin=Tin, fold_E=1, r=2, hasB=1, r_prev=3, negB=negB, u1=4, az=az, bz=bz, cz=cz, out=out, azn=azn, bzn=bzn, czn=czn, u2=1,
                outm=outm, nb=3, blocks=0)
    p = _lib.MODULUS[0]
    bad = [dict(outm=out), dict(out=az), dict(E=AZ), dict(az=short), dict(bzn=other), dict(blocks=2049), dict(nb=n + 1), dict(Tin=None), dict(r=p), dict(out=None)]
    assert R.fold_cross(**good) == _lib.OK and R.fold_cross(**dict(good, out=Tin)) == _lib.OK
    ran = 0
    for b in bad:
        assert R.fold_cross(**dict(good, **b)) == _lib.ERR_INVALID, f"vimz_test_fold_cross accepted {list(b)}"
        ran += 1
    x1, x2 = [AZ, BZ, CZ, E, E], [az, bz, cz, azn, bzn]
    assert R.fold5(x1, [0, 0, 0, 0, 4], x2, [0] * 5, [n, n, n, 4, 4], 2, 0) == _lib.OK
    assert R.fold5(x1, [0, 0, 0, 0, 3], x2, [0] * 5, [n, n, n, 4, 4], 2, 0) == _lib.ERR_INVALID, "vimz_test_fold5 accepted two overlapping ranges"
    assert R.fold5(x1, [0, 0, 1, 0, 4], x2, [0] * 5, [n, n, n, 4, 4], 2, 0) == _lib.ERR_INVALID, "vimz_test_fold5 accepted a range beyond its vector"
    ran += 2
    for x in v + [short, other]:
        x.free()
    return ran


GROUPS = (("refused", run_refused, N_REFUSED), ("fold_cross", run_fold_cross, N_FOLD_CROSS), ("fold5", run_fold5, N_FOLD5), ("fresh_cross_neg", run_fresh_neg, N_FRESH_NEG),
          ("count", run_count, N_COUNT), ("schedule", run_schedule, N_SCHEDULE))


def main(only=()):
    """only: names of groups to run alone (a developer looking at one kernel); every group is tried, and the line the test expects is printed only when every
    group of the whole list ran, in full, and passed"""
    R = Run()
    failed, counts = [], []
    try:
        for name, fn, want in GROUPS:
            if only and name not in only:
                continue
            try:
                got = fn(R)
                assert got == want, f"{name}: {got} cases ran, {want} were expected"
                counts.append(f"{name} {got}")
            except AssertionError as e:
                failed.append(name)
                print(f"FAILED {name}: {e}")
    finally:
        R.ctx.close()
    if failed:
        sys.exit(f"fold hooks: {len(failed)} group(s) failed: {' '.join(failed)}")
    print(("fold hooks ok: " if not only else "fold hooks, some groups only: ") + " ".join(counts))


if __name__ == "__main__":
    main(tuple(sys.argv[1:]))
