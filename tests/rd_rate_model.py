"""The batch and bitrate picks by distortion as plain Python integers — TEST INFRASTRUCTURE ONLY (no tests in this module).

The rules are those of include/mpeg1_hip.h ("Batch budgets and constant bitrate that pick by distortion"): the chain of a frame,
the order of all steps, the two batch forms and the bitrate walk.  Tables are S[k][f], D[k][f] (lists of lists of ints); status,
where given, is the rd table's status words, one per candidate."""
from fractions import Fraction

UNENCODABLE = 1
BEST_IN_BUDGET, SMALLEST_AT_DISTORTION = 0, 1


def running(K, status=None):
    """The candidates in the running: those whose status lacks UNENCODABLE; candidate 0 alone when every one is out."""
    ks = [k for k in range(K) if not (status is not None and int(status[k]) & UNENCODABLE)]
    return ks or [0]


def chain(s, d, ks):
    """The chain of one frame (s[k], d[k] per candidate, ks in the running): the candidate indices from v0 on."""
    v = min(ks, key=lambda k: (s[k], d[k], k))
    out = [v]
    while True:
        best = None
        for k in ks:
            if s[k] > s[v] and d[k] < d[v]:
                if best is None:
                    best = k
                    continue
                a = (d[v] - d[k]) * (s[best] - s[v])        # the cross products of the two ratios, exact
                b = (d[v] - d[best]) * (s[k] - s[v])
                if a > b or (a == b and (s[k], k) < (s[best], best)):
                    best = k
        if best is None:
            return out
        out.append(best)
        v = best


def chains(S, D, status=None):
    K, n = len(S), len(S[0])
    ks = running(K, status)
    return [chain([S[k][f] for k in range(K)], [D[k][f] for k in range(K)], ks) for f in range(n)]


def steps(S, D, ch):
    """All steps of a batch in the order they are taken: (frame, j, ds, dd), dd / ds descending, then frame, then j."""
    out = []
    for f, c in enumerate(ch):
        for j in range(1, len(c)):
            out.append((f, j, S[c[j]][f] - S[c[j - 1]][f], D[c[j - 1]][f] - D[c[j]][f]))
    out.sort(key=lambda t: (-Fraction(t[3], t[2]), t[0], t[1]))
    return out


def batch_pick(S, D, rule, limit, status=None):
    """(picks [frame] = candidate index, over) of a batch form."""
    n = len(S[0]) if S else 0
    if n == 0:
        return [], False
    ch = chains(S, D, status)
    at = [0] * n
    order = steps(S, D, ch)
    if rule == BEST_IN_BUDGET:
        total = sum(S[c[0]][f] for f, c in enumerate(ch))
        over = total > limit
        if not over:
            for f, j, ds, _ in order:
                if total + ds > limit:
                    break
                total += ds
                at[f] = j
    else:
        total = sum(D[c[0]][f] for f, c in enumerate(ch))
        for f, j, _, dd in order:
            if total <= limit:
                break
            total -= dd
            at[f] = j
        over = total > limit
    return [ch[f][at[f]] for f in range(n)], over


def bitrate_walk(S, D, rate, cap, level, status=None):
    """(picks, frames over their level, the level after the batch) of the bitrate form."""
    K, n = len(S), (len(S[0]) if S else 0)
    ks = running(K, status)
    L = min(level, cap)
    picks, over = [], []
    for f in range(n):
        fit = [k for k in ks if S[k][f] <= L]
        if fit:
            k = min(fit, key=lambda k: (D[k][f], S[k][f], k))
        else:
            k = min(ks, key=lambda k: (S[k][f], k))
            over.append(f)
        picks.append(k)
        L = min(cap, L - S[k][f] + rate)
    return picks, over, L


def batch_byte_rule(S, limit):
    """The picks of m1v_encode_batch_budget_device (the largest level that fits, then the cheapest upgrades): (picks, over)."""
    K, n = len(S), len(S[0])
    T = [sum(S[k]) for k in range(K)]
    fits = [k for k in range(K) if T[k] <= limit]
    if not fits:
        return [0] * n, True
    top = fits[-1]
    if top == K - 1:
        return [top] * n, False
    d = [S[top + 1][f] - S[top][f] for f in range(n)]
    picks = [top + 1 if d[f] <= 0 else top for f in range(n)]
    room = limit - T[top] + sum(-x for x in d if x < 0)
    for x, f in sorted((d[f], f) for f in range(n) if d[f] > 0):
        if x > room:
            break
        room -= x
        picks[f] = top + 1
    return picks, False


def bitrate_byte_rule(S, rate, cap, level):
    """The picks of m1v_encode_cbr_device (the largest candidate that fits the level, else candidate 0): (picks, over, level)."""
    K, n = len(S), len(S[0])
    L = min(level, cap)
    picks, over = [], []
    for f in range(n):
        fit = [k for k in range(K) if S[k][f] <= L]
        k = fit[-1] if fit else 0
        if not fit:
            over.append(f)
        picks.append(k)
        L = min(cap, L - S[k][f] + rate)
    return picks, over, L
