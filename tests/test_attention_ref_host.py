"""No GPU: the inputs of tests/test_gpu_attention.py satisfy the conditions its tests rely on, for every case it parametrizes (the
branch each case reaches, designated-key weight and coverage, the score cap, padding scores, where the row maximum moves), the
float64 reference agrees with a masked torch.softmax, and the per-row bound 2^-7 A of tests/attention_ref.py separates a correct
tile-wise online softmax with bf16 P from six that are wrong on purpose.  Ratios quoted below are err / (3 x 2^-9 A); the bound is
4/3 on that scale."""
import math

import pytest
import torch

from tests import attention_ref as R

CASES = R.cases()
IDS = [R.case_id(c) for c in CASES]


def rounded(name, c):
    q, k, v, scale = R.build(name, c)
    return R.q16(q), R.q16(k), R.q16(v), scale


def args(c):
    return c.B, c.Tq, c.Tk, c.heads, c.dh


def test_every_case_reaches_the_branch_it_names():
    assert len(set(IDS)) == len(IDS)
    for c in CASES:
        assert R.branch_of(c.Tq, c.Tk, c.dh, c.causal) == c.branch, R.case_id(c)
    assert {c.branch for c in CASES} == set(R.TILE)
    assert {c.branch for c in CASES if c.separate} == set(R.TILE) and sum(c.separate for c in CASES) == len(R.TILE)
    for br in ('G', 'C'):
        assert {c.dh for c in CASES if c.branch == br} == set(R.DHS)
    wide_k = [c for c in CASES if c.branch == 'K' and c.Tq >= 1024 and c.Tk >= 1024]
    assert len(wide_k) == 1 and wide_k[0].dh == 64
    # designated: everywhere at dh >= 32, at dh 8 and 16 on the non-wide branches
    for c in CASES:
        assert ('designated' in R.sets_of(c)) == (c.dh >= 32 or c.branch not in ('W0', 'W1'))
        assert ('ascending' in R.sets_of(c)) == (c.Tk > c.tile) == ('descending' in R.sets_of(c))


@pytest.mark.parametrize('c', CASES, ids=IDS)
def test_builder_properties(c):
    B, Tq, Tk, heads, dh = args(c)
    vis = R.visible(Tq, Tk, c.causal)
    for name in R.sets_of(c):
        q, k, v, scale = rounded(name, c)
        what = f'{R.case_id(c)} {name}'
        assert q.shape == (B * Tq, heads * dh) and k.shape == v.shape == (B * Tk, heads * dh)
        vh = v.view(B, Tk, heads, dh)
        assert torch.equal(vh[0, :, 0, 0], R.q16(torch.arange(Tk) / Tk))
        assert all(torch.all(vh[b, :, h, 1] == b * heads + h + 1) for b in range(B) for h in range(heads))
        for pre in ([False, True] if c.branch == 'D' else [False]):          # (the dh-40 long path rounds the scaled queries)
            p, s = R.weights(q, k, B, Tq, Tk, heads, dh, scale, c.causal, pre)
            raw = R.scores_log2(q, k, B, Tq, Tk, heads, dh, scale, pre)
            assert raw.abs().max() <= R.SCORE_CAP, f'{what}: score cap, {raw.abs().max():.1f}'
            if name == 'designated':
                key = R.designated_keys(B, Tq, Tk, heads, c.tile, c.causal, R.build_seed(name, c))
                w = p.gather(-1, key[..., None])[..., 0]
                assert w.min() >= 0.95, f'{what}: designated weight {w.min():.3f}'
                assert bool(vis[torch.arange(Tq), key].all())
                must = R.must_cover(Tk, c.tile)
                for b in range(B):
                    for h in range(heads):
                        got = set(key[b, h].tolist())
                        if c.causal:
                            assert got >= set(range(min(Tq, Tk)))
                        elif Tq >= Tk:
                            assert got == set(range(Tk))
                        elif Tq >= len(must):
                            assert got >= set(must) and {0, Tk - 1} <= set(must)
                if not c.causal and Tq < len(R.must_cover(Tk, c.tile)) and Tq < Tk:          # one query: the first of the list, between them
                    allk = set(key.flatten().tolist())
                    assert Tk - 1 in allk and 0 in allk
            elif name == 'padding_would_win':
                nat = raw / R.LOG2E
                assert nat.max() <= -15.0 and nat.min() >= -25.0, f'{what}: {nat.min():.1f} .. {nat.max():.1f}'
            elif name == 'uniform':
                assert raw.abs().max() == 0
            elif name in ('ascending', 'descending'):
                nt = (Tk + c.tile - 1) // c.tile
                tmax = torch.stack([s[..., t * c.tile:(t + 1) * c.tile].amax(-1) for t in range(nt)], -1)      # [B, heads, Tq, nt]
                if c.causal:
                    tmax = tmax[:, :, Tk - 1:]                     # (rows that see every tile)
                step = tmax[..., 1:] - tmax[..., :-1]
                if step.numel() == 0:                              # (causal with fewer queries than keys: no row sees a second tile whole)
                    continue
                if name == 'ascending':
                    assert step.min() > 0, f'{what}: the maximum does not move in every tile ({step.min():.2f})'
                    if nt >= 3:
                        assert (step > 6).any(-1).all() and (step < 6).any(-1).all(), f'{what}: steps on one side of 6'
                else:
                    assert step.max() < 0, f'{what}: the maximum moves after tile 0 ({step.max():.2f})'


def test_must_cover_holds_the_neighbours_of_every_boundary():
    for Tk, tile in ((200, 64), (1153, 128), (2049, 64), (17, 64)):
        must = R.must_cover(Tk, tile)
        assert must[0] == Tk - 1 and 0 in must
        for step in (16, 32, tile):
            for m in range(step, Tk, step):
                assert m - 1 in must and (m + 1 in must or m + 1 >= Tk)


@pytest.mark.parametrize('Tq,Tk', [(77, 77), (100, 64), (64, 100), (1, 1), (130, 130)])
def test_causal_reference_is_a_masked_torch_softmax(Tq, Tk):
    c = R.Case('K', 2, Tq, Tk, 2, 40, 1, 64, False)
    for name in ('soft', 'hard'):
        q, k, v, scale = rounded(name, c)
        B, _, _, heads, dh = args(c)
        out, A = R.ref(q, k, v, B, Tq, Tk, heads, dh, scale, causal=True)
        qh, kh, vh = (t.double().view(B, -1, heads, dh).transpose(1, 2) for t in (q, k, v))
        i, j = torch.arange(Tq)[:, None], torch.arange(Tk)[None, :]
        mask = j > torch.clamp(i, max=Tk - 1)                        # query i sees keys 0 .. min(i, Tk - 1)
        sc = (qh @ kh.transpose(-1, -2) * scale).masked_fill(mask, -math.inf)
        want = (torch.softmax(sc, -1) @ vh).transpose(1, 2).reshape(B * Tq, heads * dh)
        # (1e-6, not 1e-12: the reference forms scale * log2(e) in fp32, as the launcher does)
        assert (out - want).abs().max() <= 1e-6 * max(1.0, want.abs().max().item())
        assert (A >= out.abs().view(B * Tq, heads, dh).amax(-1) - 1e-12).all()


# ---- the bound separates right from wrong ----------------------------------------------------------------------------------------------
# (case, emulation mode): the generic kernel at 130 keys, the long kernels at 1153 and 2049 keys, the dh-40 long path, causal
EMU = {
    'G130': (R.Case('G', 2, 100, 130, 2, 40, 0, 64, False), 'plain'),
    'W1153': (R.Case('W0', 1, 1040, 1153, 2, 64, 0, 64, False), 'plain'),
    'W2049': (R.Case('W1', 1, 1040, 2049, 2, 64, 0, 64, False), 'msum'),
    'D1025': (R.Case('D', 1, 1040, 1025, 2, 40, 0, 128, False), 'dma'),
    'D1153': (R.Case('D', 1, 1040, 1153, 2, 40, 0, 128, False), 'dma'),
    'D2049': (R.Case('D', 1, 1040, 2049, 2, 40, 0, 128, False), 'dma'),
    'K130': (R.Case('K', 2, 130, 130, 2, 64, 1, 64, False), 'plain'),
}
_cache = {}


def scaled_ratio(tag, name, mutant=None, mtile=1):
    """worst err / (3 x 2^-9 A) over (row, head) of the emulation against the float64 reference (computed once per (case, set))."""
    c, mode = EMU[tag]
    if (tag, name) not in _cache:
        q, k, v, scale = rounded(name, c)
        _cache[tag, name] = (q, k, v, scale) + R.ref(q, k, v, *args(c), scale, c.causal, prescale=mode == 'dma')
    q, k, v, scale, want, A = _cache[tag, name]
    out = R.emulate(q, k, v, c, scale, mode, mutant, mtile)
    r = R.ratios(out, want, A, c.heads, c.dh)
    assert torch.isfinite(r).all()
    return r.max().item() * 4.0 / 3.0


FAILS = 4.0 / 3.0


@pytest.mark.parametrize('tag', list(EMU))
def test_correct_emulation_is_within_the_bound_on_every_set(tag):
    c, _ = EMU[tag]
    for name in R.sets_of(c):
        r = scaled_ratio(tag, name)
        print(f'{tag} {name}: correct emulation {r:.2f} of 3 x 2^-9 A')
        assert r <= FAILS, f'{tag} {name}: {r:.2f}'


@pytest.mark.parametrize('tag', ['G130', 'W1153', 'W2049'])
def test_dropped_tile_and_skipped_rescale_fail(tag):
    """norescale: tile 1 on random scores (the maximum moves there in most rows), the last tile on ascending ones (everything before it
    is then overweighted by the last step).  droptile on flat weights is arithmetic on the ramp channel: dropping the 64 keys of tile 1
    moves the mean of j / Tk by (0.5 - 96 / Tk) 64 / (Tk - 64), and A = 1 where the code channel is 1: 4.7 x (3 x 2^-9 A) at 1153
    keys but 2.6 at 2049, twice the bound and short of 3; a 128-key tile of the dh-40 path gives 5 there (D2049 below)."""
    u = scaled_ratio(tag, 'uniform', 'droptile')
    print(f'{tag} uniform: droptile {u:.1f}')
    assert u >= (3.0 if tag != 'W2049' else 2.0)
    for name in ('soft', 'hard'):
        a, b = scaled_ratio(tag, name, 'droptile'), scaled_ratio(tag, name, 'norescale')
        print(f'{tag} {name}: droptile {a:.1f}, norescale {b:.1f}')
        assert a >= 7.0 and b >= 7.0
    a = scaled_ratio(tag, 'ascending', 'norescale', mtile=-1)
    print(f'{tag} ascending: norescale {a:.1f}')
    assert a > FAILS


@pytest.mark.parametrize('tag', ['G130', 'W1153', 'W2049', 'D1153'])
def test_dropped_last_key_needs_the_designated_set(tag):
    u, d = scaled_ratio(tag, 'uniform', 'droplast'), scaled_ratio(tag, 'designated', 'droplast')
    print(f'{tag}: droplast uniform {u:.2f}, designated {d:.1f}')
    assert d > FAILS
    if EMU[tag][0].Tk >= 1024:
        assert u <= FAILS          # flat weights hide one key of a thousand


@pytest.mark.parametrize('tag', ['D1025', 'D1153', 'D2049'])
def test_lazy_reference_mutants_fail(tag):
    """The dh-40 long path: a skipped rescale shows where the reference moves (ascending; the last even tile: a step of 9 - after a
    step of 3 the lazy reference stays and there is no rescale to skip), an unmasked clamp on flat weights."""
    c = EMU[tag][0]
    a = scaled_ratio(tag, 'ascending', 'norescale', mtile=(((c.Tk + c.tile - 1) // c.tile - 1) // 2) * 2)
    u = scaled_ratio(tag, 'uniform', 'clamp')
    t = scaled_ratio(tag, 'uniform', 'droptile')
    print(f'{tag}: norescale ascending {a:.1f}, clamp uniform {u:.1f}, droptile uniform {t:.1f}')
    assert a > FAILS and u > FAILS and t >= 3.0


def test_swapped_heads_and_ignored_causal_limit_fail():
    for tag in ('G130', 'W2049', 'D1153'):
        for name in ('uniform', 'designated'):
            r = scaled_ratio(tag, name, 'swapheads')
            print(f'{tag} {name}: swapheads {r:.1f}')
            assert r > FAILS
    for name in ('uniform', 'soft', 'hard'):
        r = scaled_ratio('K130', name, 'nocausal')
        print(f'K130 {name}: nocausal {r:.1f}')
        assert r > FAILS


def test_prescaling_gap_of_the_dh40_long_path():
    """Exact against emulated-query float64 reference, CPU only: what the kernel's documented input rounding (AttnCfg::OFFS) costs.
    Printed for the header of tests/test_gpu_attention.py; it carries no assertion on the kernel."""
    for Tk in (130, 1153, 2049):
        c = R.Case('D', 1, 1040, Tk, 2, 40, 0, 128, False)
        for name in ('soft', 'hard'):
            q, k, v, scale = rounded(name, c)
            exact, A = R.ref(q, k, v, *args(c), scale)
            emu, _ = R.ref(q, k, v, *args(c), scale, prescale=True)
            gap = (R.row_err(emu, exact, c.heads, c.dh) / A).max().item()
            rl2 = ((emu - exact).norm() / exact.norm()).item()
            print(f'pre-scaling gap Tk={Tk} {name}: worst row {gap:.2e} A, rel-L2 {rl2:.2e}')
            assert gap <= 2.0 ** -5          # two bf16 roundings of a score of a few units: far from any fault's size
