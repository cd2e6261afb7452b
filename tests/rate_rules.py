"""The budget rules of include/mpeg1_hip.h as plain Python on a size table s[k][f]: what tests/test_rate_abi.py holds the header's
wording to, and what the GPU tests expect of the batch-budget and constant-bitrate encodes of every input layout."""


def batch_rule(s, B):
    """s[k][f]: record size of frame f at candidate k.  Returns (picks, over_budget)."""
    K, n = len(s), len(s[0])
    T = [sum(s[k]) for k in range(K)]
    fit = [k for k in range(K) if T[k] <= B]
    if not fit:
        return [0] * n, True
    k = fit[-1]
    if k == K - 1:
        return [k] * n, False
    pick = [k] * n
    d = [s[k + 1][f] - s[k][f] for f in range(n)]
    room = B - T[k]
    for f in range(n):
        if d[f] <= 0:
            pick[f], room = k + 1, room - d[f]
    for f in sorted((f for f in range(n) if d[f] > 0), key=lambda f: (d[f], f)):
        if d[f] > room:
            break
        pick[f], room = k + 1, room - d[f]
    return pick, False


def cbr_rule(s, r, C, L):
    """Returns (picks, frames that fit nothing, level after the batch)."""
    K, n = len(s), len(s[0])
    L = min(L, C)
    pick, over = [], []
    for f in range(n):
        fit = [k for k in range(K) if s[k][f] <= L]
        k = fit[-1] if fit else 0
        if not fit:
            over.append(f)
        L = min(C, L - s[k][f] + r)
        pick.append(k)
    return pick, over, L


def batch_rule_prefix_test(s, B):
    """The form k_rate_pick evaluates: frame f with d[f] > 0 goes up iff the positive d[j] with (d[j], j) <= (d[f], f) sum to
    at most the room left after the free upgrades."""
    K, n = len(s), len(s[0])
    T = [sum(s[k]) for k in range(K)]
    fit = [k for k in range(K) if T[k] <= B]
    if not fit or fit[-1] == K - 1:
        return batch_rule(s, B)
    k = fit[-1]
    d = [s[k + 1][f] - s[k][f] for f in range(n)]
    room = B - T[k] + sum(-x for x in d if x <= 0)
    pick = []
    for f in range(n):
        prefix = sum(d[j] for j in range(n) if d[j] > 0 and (d[j], j) <= (d[f], f))
        pick.append(k + 1 if d[f] <= 0 or prefix <= room else k)
    return pick, False
