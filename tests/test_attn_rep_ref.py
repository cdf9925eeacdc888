"""attn_rep_ref.py without a GPU: the inputs and the bound of test_gpu_attn_rep_ops.py are sound before any kernel is involved -- on
every random case the GPU test runs, the faithful emulation of the kernel's rounding points and a plain float32 run of the reference
both stay inside the derived bound -- and the exact cases have teeth: every deliberate mistake the emulation can make (a dropped
last key, a dropped slice, the next kv head, a row off by one under two rows per wave, an unmasked stale tail) fails a named exact
case bit for bit."""
import numpy as np
import pytest

import attn_cases as ac
import attn_rep_ref as ar


@pytest.mark.parametrize("d", [64, 128])
def test_random_cases_are_inside_the_bound(d):
    """the faithful emulation and a float32 run of the reference, on the cases and the row counts of the GPU test"""
    worst = {"emulation": (0.0, ""), "float32 reference": (0.0, "")}
    for H, Hkv in ar.layouts(d):
        w = ar.random_w(d, H, Hkv)
        ns = ar.n_list(d, H, Hkv)
        for S, cap in ar.s_cases(H, Hkv, d):
            q, k, v = ar.random_inputs(d, H, Hkv, S)
            ref, B, _, _ = ar.bound(q, k, v, w, S, H, Hkv, d)
            runs = {"emulation": ar.emulate(q, k, v, w, S, H, Hkv, d, pad=ar.STALE),
                    "float32 reference": ar.reference(q, k, v, w, S, H, Hkv, d, dtype=np.float32)[0]}
            for what, got in runs.items():
                assert np.isfinite(got).all()
                ratio = np.abs(got.astype(np.float64) - ref) / B
                for N in ns:                                         # a case with N rows is the first N rows
                    r = float(ratio[:N].max())
                    tag = "d=%d H=%d Hkv=%d S=%d N=%d" % (d, H, Hkv, S, N)
                    worst[what] = max(worst[what], (r, tag))
                    assert r <= 1.0, "%s, %s: err / bound %.3f" % (tag, what, r)
    for what, (r, tag) in worst.items():
        print("d=%d %s: worst err / bound %.4f (%s)" % (d, what, r, tag))


def _emulated_forms(sel, S, H, Hkv, d, N, seed, mistake, dropped_slice=1):
    """[(form name, index of the first wrong element or None, its description)] of one selector under one mistake"""
    out = []
    for name, v, w, want, where in ar.exact_forms(sel, N, seed):
        got = ar.emulate(sel.q.reshape(-1), sel.k.reshape(S + H // Hkv, -1), v.reshape(S + H // Hkv, -1), w, S, H, Hkv, d, pad=ar.STALE,
                         mistake=mistake, dropped_slice=dropped_slice)
        bad = ar.first_difference(got, want)
        out.append((name, bad, where(bad) if bad is not None else ""))
    return out


# (d, H, Hkv, S, N): small shapes of the GPU test's lists; N = 2049 is odd and runs two rows per wave
TEETH = [(64, 6, 2, 129, 9), (128, 4, 1, 257, 512), (64, 12, 4, 65, 2049), (64, 8, 8, 33, 7)]


@pytest.mark.parametrize("d,H,Hkv,S,N", TEETH)
def test_the_faithful_emulation_passes_every_exact_case(d, H, Hkv, S, N):
    for j, sel in enumerate(ar.selectors(S + d + H, S, H, Hkv, d)):
        for name, bad, where in _emulated_forms(sel, S, H, Hkv, d, N, j, None):
            assert bad is None, "%s, selector %d: row %d differs (%s)" % (name, j, bad, where)


def test_every_deliberate_mistake_fails_an_exact_case():
    """... and which one: printed per mistake and exact-case family"""
    caught = {}

    def run(mistake, d, H, Hkv, S, N, only=None, dropped_slice=1):
        sels = ar.selectors(S + d + H, S, H, Hkv, d)
        for j, sel in enumerate(sels):
            if only is not None and not only(sel):
                continue
            for name, bad, where in _emulated_forms(sel, S, H, Hkv, d, N, j, mistake, dropped_slice):
                if bad is not None:
                    caught.setdefault((mistake, name), "d=%d H=%d Hkv=%d S=%d N=%d selector %d: row %d, %s" % (d, H, Hkv, S, N, j, bad, where))
        return len(sels)

    # the last key: a selector whose targets include key S - 1
    run("drop_last_key", 64, 6, 2, 129, 384, only=lambda sel: (sel.pi == 128).any())
    # slice 1 of 4 dropped: a selector in which that slice owns a target (tiles 1, 5, ...: keys 32..63)
    owns = lambda sel: any(ar.owner_slice(int(p), 2) == 1 for p in sel.pi.ravel())
    assert run("drop_slice", 64, 6, 2, 129, 384, only=owns, dropped_slice=1) > 0
    run("kv_head", 64, 6, 2, 129, 384)
    run("no_mask", 64, 6, 2, 129, 384)
    # two rows per wave and an odd row count
    assert ar.rpw(2049) == 2 and 2049 % 2 == 1
    run("row", 64, 12, 4, 65, 2049)
    for mistake in ar.MISTAKES:
        for form in ("sign-select", "integers"):
            print("%-14s %-11s %s" % (mistake, form, caught.get((mistake, form), "not caught")))
        assert (mistake, "sign-select") in caught or (mistake, "integers") in caught, "no exact case fails under the mistake %r" % mistake
    # a dropped slice that owns no target of a selector leaves that selector exact: the assertion above is about ownership
    sels = ar.selectors(129 + 64 + 6, 129, 6, 2, 64)
    free = [j for j, sel in enumerate(sels) if not any(ar.owner_slice(int(p), 2) == 1 for p in sel.pi.ravel())]
    for j in free[:1]:
        assert all(bad is None for _, bad, _ in _emulated_forms(sels[j], 129, 6, 2, 64, 9, j, "drop_slice", 1))
    # the row mistake is only there with two rows per wave: N = 2048 runs one
    assert all(bad is None for _, bad, _ in _emulated_forms(ar.selectors(65 + 64 + 12, 65, 12, 4, 64)[0], 65, 12, 4, 64, 2048, 0, "row"))


@pytest.mark.parametrize("d", [64, 128])
def test_selector_margins_targets_and_decoys(d):
    """every selector case of the GPU test: the score gap, every target taken, every decoy class present"""
    for H, Hkv in ar.layouts(d):
        G = H // Hkv
        for S, cap in ar.s_cases(H, Hkv, d):
            sels = ar.selectors(ar.random_seed(d, H, Hkv, S), S, H, Hkv, d)
            want = ar.targets(S, Hkv, d)
            assert {0, S - 1} <= set(want)
            assert set(int(p) for sel in sels for p in sel.pi.ravel()) == set(want), (d, H, Hkv, S)
            for sel in sels:
                worst, ok = sel.margin()
                assert ok and worst < -ac.GAP
                assert set(sel.decoys) == ac.decode_decoy_classes(S, Hkv)
                assert sel.k.shape[0] == S + G and S + G <= cap
