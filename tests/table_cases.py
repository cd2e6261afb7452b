"""The case tables and mixed sequences of the size-table and rate tests, which the tests of the other input layouts (RGBA,
surfaces, planes) run through their own kernels: RGB_CASES and Mixed (tests/test_gpu_size_table.py), RGBA_CASES
(tests/test_gpu_rgba_table.py), SEQUENCE and RateMixed (tests/test_gpu_rate.py), MATRIX (tests/test_gpu_surface.py)."""
import numpy as np

from gpu_calls import _mixed_frames, _oracle, _oracle_sizes
from rate_rules import batch_rule, cbr_rule

RGB_CASES = {
    # name: (W, H, Q, mode, n, amps, qualities)
    "cif_full_k8": (352, 288, 12, "full", 4, (4, 40, 256, 120), (1, 2, 3, 5, 7, 9, 11, 12)),
    "cif_strict_k1": (352, 288, 12, "strict", 3, (4, 40, 256), (7,)),
    "q90_wide_staging": (352, 288, 90, "full", 3, (4, 40, 20), (1, 20, 60, 76, 77, 85, 90)),
    "q90_narrow_only": (352, 288, 90, "full", 2, (40, 256), (10, 50, 76)),
    "partial_tiles_366x216": (366, 216, 12, "full", 3, (4, 40, 256), (1, 6, 12)),
    "tiny_105x49": (105, 49, 12, "full", 4, (4, 40, 256, 120), (1, 12)),
    "uhd_one_frame": (3840, 2160, 12, "full", 1, (256,), (1, 5, 12)),
}


CANDS = (2, 4, 8, 12)


def _rule(table, budgets):
    """The largest candidate whose record fits, else the smallest: (chosen, over-budget frames)."""
    chosen, over = [], []
    for f, cap in enumerate(budgets):
        fits = [c for c in CANDS if table[c][f] <= cap]
        chosen.append(fits[-1] if fits else CANDS[0])
        if not fits:
            over.append(f)
    return chosen, over


class Mixed:
    """Calls of every kind on one encoder, the size table among them; each call's expected output is computed from the oracle
    at check time (the pattern of tests/test_gpu_quality.py)."""

    def __init__(self, torch, orc, enc, seed):
        self.torch, self.orc, self.enc = torch, orc, enc
        self.rng = np.random.default_rng(seed)
        self.pending = []
        self.first = 200

    def call(self, kind, n):
        torch, enc, orc = self.torch, self.enc, self.orc
        rgb = _mixed_frames(self.rng, n, enc.width, enc.height, enc.channels)
        dev = torch.from_numpy(rgb).cuda()
        self.first += 29
        Q = enc.quality_factor
        if kind == "plain":
            self.pending.append((kind, rgb, self.first, [Q] * n, dev, enc.encode(dev, self.first)))
        elif kind == "quality":
            qs = [int(x) for x in self.rng.integers(1, Q + 1, n)]
            self.pending.append((kind, rgb, self.first, qs, dev, enc.encode(dev, self.first, quality=qs)))
        elif kind == "probe":
            qs = [int(x) for x in self.rng.integers(1, Q + 1, n)]
            self.pending.append((kind, rgb, self.first, qs, dev, enc.frame_sizes(dev, quality=qs)))
        elif kind == "table":
            k = int(self.rng.integers(1, 9))
            quals = sorted(int(x) for x in self.rng.choice(np.arange(1, Q + 1), min(k, Q), replace=False))
            self.pending.append((kind, rgb, self.first, quals, dev, enc.frame_size_table(dev, quals)))
        else:                                    # synchronous: checked at once against the rule on the oracle's sizes
            table = {c: _oracle(orc, rgb, self.first, [c] * n, orc.MODE_FULL, enc.channels)[1] for c in CANDS}
            budget = sorted(table[8])[0]
            chosen, over = _rule(table, [budget] * n)
            got, sizes, ch, ov = enc.encode_to_budget(dev, budget, CANDS, first_frame_index=self.first)
            want, wsizes = _oracle(orc, rgb, self.first, chosen, orc.MODE_FULL, enc.channels)
            assert (ch, ov, sizes, got) == (chosen, over, wsizes, want), ("budget", n)

    def check(self, what):
        self.enc.flush()
        self.torch.cuda.synchronize()
        for k, (kind, rgb, first, qs, _, res) in enumerate(self.pending):
            n = rgb.shape[0]
            if kind == "table":
                want = [_oracle_sizes(self.orc, rgb, self.orc.MODE_FULL, q, self.enc.channels) for q in qs]
                assert res.cpu().numpy().tolist() == want, (what, k, kind, qs)
                continue
            want, wsizes = _oracle(self.orc, rgb, first, qs, self.orc.MODE_FULL, self.enc.channels)
            if kind == "probe":
                assert [int(s) for s in res[:n].cpu()] == wsizes, (what, k, kind)
                continue
            out, sizes, meta = res
            total, status = (int(x) for x in meta.cpu())
            assert status == 0, (what, k, kind, status)
            assert [int(s) for s in sizes[:n].cpu()] == wsizes, (what, k, kind)
            assert out[:total].cpu().numpy().tobytes() == want, (what, k, kind)
        self.pending = []


# the cases of tests/test_gpu_size_table.py, a geometry whose encodes take the strip kernel (9 macroblock rows: 54 blocks per
# strip), and a width whose last tile column holds an odd number of strips (11 = 8 + 3)
RGBA_CASES = dict(RGB_CASES)
RGBA_CASES["strip_kernel_352x144"] = (352, 144, 12, "full", 4, (4, 40, 256, 120), (1, 3, 8, 12))
RGBA_CASES["odd_last_column_176x208"] = (176, 208, 12, "full", 3, (4, 256, 40), (2, 7, 12))


def _table(orc, rgb, cands, channels=3):
    return [_oracle_sizes(orc, rgb, orc.MODE_FULL, c, channels) for c in cands]


RCANDS = (3, 7, 12)


class RateMixed(Mixed):
    """Mixed (tests/test_gpu_size_table.py) with batch-budget and bitrate calls, checked at once against the rules."""

    def __init__(self, torch, orc, enc, seed):
        super().__init__(torch, orc, enc, seed)
        self.level = torch.full((1,), 123456, dtype=torch.int64, device="cuda")
        self.level_host = 123456

    def call(self, kind, n):
        if kind not in ("batch", "cbr"):
            return super().call(kind, n)
        torch, enc, orc = self.torch, self.enc, self.orc
        rgb = _mixed_frames(self.rng, n, enc.width, enc.height, enc.channels)
        dev = torch.from_numpy(rgb).cuda()
        self.first += 29
        s = _table(orc, rgb, RCANDS, enc.channels)
        if kind == "batch":
            B = (sum(s[0]) + sum(s[1])) // 2
            pick, over = batch_rule(s, B)
            got, sizes, ch, ov = enc.encode_to_batch_budget(dev, B, RCANDS, first_frame_index=self.first)
        else:
            r = sorted(s[1])[n // 2]
            pick, over, self.level_host = cbr_rule(s, r, 3 * r, self.level_host)
            got, sizes, ch, ov = enc.encode_at_bitrate(dev, r, 3 * r, RCANDS, self.level, first_frame_index=self.first)
            assert int(self.level.cpu()[0]) == self.level_host, (int(self.level.cpu()[0]), self.level_host)
        chosen = [RCANDS[k] for k in pick]
        want, wsizes = _oracle(orc, rgb, self.first, chosen, orc.MODE_FULL, enc.channels)
        assert (ch, ov, sizes, got) == (chosen, over, wsizes, want), (kind, n)


SEQUENCE = (("plain", 5), ("batch", 4), ("table", 3), ("cbr", 5), ("probe", 3), ("quality", 5), ("cbr", 2), ("budget", 2),
            ("batch", 5), ("table", 1), ("plain", 5))


# geometry and content of the cases of tests/test_gpu_size_table.py and test_gpu_rgba_table.py (wide staging, partial tiles,
# an odd last tile column, the strict region, a 4K frame), an even tiny picture in place of the odd-width one (for which every
# surface layout is an argument error: test_odd_width_keeps_the_default_layout), and a 1080p pair
MATRIX = {k: v for k, v in {**RGB_CASES, **RGBA_CASES}.items() if k != "tiny_105x49"}
MATRIX["tiny_96x48"] = (96, 48, 12, "full", 4, (4, 40, 256, 120), (1, 12))
MATRIX["hd_pair"] = (1920, 1080, 12, "full", 2, (256, 40), (3, 12))
