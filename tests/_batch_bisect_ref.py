"""A plain-Python model of the bisection planner of the two batch verifiers (vimz_amd/csrc/batch_bisect.hpp), written from the rule and not from the header:

  * a refused subset of at most `leaf` members goes to the single verifier;
  * a larger refused subset [lo, hi) is split into L = [lo, lo + ceil((hi - lo) / 2)) and R, the rest; L is asked on the sides its parent was refused on; if it
    holds on all of them its members are accepted and R is refused by implication with the parent's sides and no evaluation; otherwise R is asked too;
  * level by level over all chunks: every L of a level, then the R subsets that need it.

A member's equation on a side fails iff the member is bad on that side, and a subset's equation on a side fails iff some member of it is bad on that side (what
random multipliers give, up to 2^-128).  Test infrastructure; no GPU."""


def chunks_of(n, chunk):
    return [(lo, min(n, lo + chunk)) for lo in range(0, n, chunk)]


def plan(roots, bad, leaf):
    """roots: [(lo, hi)] chunks; bad: {member: mask of the sides it fails on}; leaf >= 1.  -> {"asked": [(lo, hi, sides)] in order, "singles": [(lo, hi, sides)] in
    order, "stats": [chunks refused, side equations evaluated, single verifications, members accepted by a subset equation], "subsets": subsets asked}"""
    leaf = max(1, leaf)

    def fails(lo, hi):
        m = 0
        for i in range(lo, hi):
            m |= bad.get(i, 0)
        return m

    frontier = [(lo, hi, fails(lo, hi)) for lo, hi in roots if fails(lo, hi)]
    asked, singles, accepted = [], [], 0
    refused = len(frontier)
    while frontier:
        work = []
        for nd in frontier:
            if nd[1] - nd[0] <= leaf:
                singles.append(nd)
            else:
                work.append(nd)
        mids = [lo + (hi - lo + 1) // 2 for lo, hi, _ in work]
        left = []
        for (lo, hi, sides), m in zip(work, mids):
            asked.append((lo, m, sides))
            left.append(sides & fails(lo, m))
        right = []
        for (lo, hi, sides), m, lf in zip(work, mids, left):
            if lf:
                asked.append((m, hi, sides))
                right.append(sides & fails(m, hi))
            else:
                right.append(None)
        frontier = []
        for (lo, hi, sides), m, lf, rt in zip(work, mids, left, right):
            if not lf:
                accepted += m - lo
                frontier.append((m, hi, sides))
                continue
            frontier.append((lo, m, lf))
            if rt:
                frontier.append((m, hi, rt))
            else:
                accepted += hi - m
    n_single = sum(hi - lo for lo, hi, _ in singles)
    return {"asked": asked, "singles": singles, "subsets": len(asked),
            "stats": [refused, sum(bin(s).count("1") for _, _, s in asked), n_single, accepted]}


def stats_without_bisection(roots, bad):
    """the parent's loop: every member of a refused chunk goes to the single verifier"""
    ref = [(lo, hi) for lo, hi in roots if any(bad.get(i, 0) for i in range(lo, hi))]
    return [len(ref), 0, sum(hi - lo for lo, hi in ref), 0]
