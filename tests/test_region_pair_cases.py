"""The case table of tests/region_pair_cases.py against the branches of csrc/region_min.hip (CPU only): if a kernel
constant moves, or the table is edited, and a branch is no longer reached, this fails rather than the GPU tests quietly
covering less.  The thresholds are restated here as plain numbers on purpose."""
import numpy as np

import region_pair_cases as rc

TILE = 1024          # kTile: columns staged in LDS per pass of region_pair_min_kernel
WORDS = 16           # kWords: mask words of a row preloaded into registers (rows of up to 16 * 32 = 512 columns)
ROWS_TILE = 256      # kRowsTile: columns staged per pass of region_pair_rows_kernel
ROUND_ROWS = 256     # 64 rows per block x kPairWaves = 4 wavefronts: rows of one round of region_pair_min_kernel
COL_SPLIT = 4        # kPairColSplit: column quarters of a pair in region_pair_rows_kernel, cut at whole 32-bit words
SHARES = 16          # kPairShares: a body's selected pairs are dealt over this many shares


def quarters(n2):
    words = (n2 + 31) // 32
    return [(min(n2, words * zc // COL_SPLIT * 32), min(n2, words * (zc + 1) // COL_SPLIT * 32)) for zc in range(COL_SPLIT)]


def test_table_is_the_issue_s():
    names, lists = rc.regions()
    assert [len(r) for r in lists[:-1]] == list(rc.SIZES) and names[-1] == 'N0'
    assert all(len(set(r.tolist())) == len(r) for r in lists)
    assert any((np.diff(r) < 0).any() for r in lists)             # region-list order is not vertex order
    assert len(rc.PAIR_NAMES) == 24 and len(set(rc.PAIR_NAMES)) == 24
    for a, b in rc.PAIR_NAMES:                                     # both orders wherever the two regions differ
        assert (b, a) in rc.PAIR_NAMES
    gm, v = rc.mask(), rc.vertices('raw')
    assert not gm.diagonal().any() and np.array_equal(gm, gm.T) and v.shape == (3, 1602, 3) and v.dtype == np.float32
    grid = rc.vertices('grid').astype(np.float64) / rc.GRID
    assert np.array_equal(grid, np.round(grid)) and np.abs(rc.vertices('grid') - v).max() <= rc.GRID / 2


def test_sizes_reach_every_branch():
    sizes = rc.pair_sizes()
    n1s, n2s = [a for a, _ in sizes], [b for _, b in sizes]
    assert any(n2 > TILE for n2 in n2s)                                     # several LDS passes
    assert any(n2 > TILE and n1 > ROUND_ROWS for n1, n2 in sizes)           # ... restaged for a second round of row blocks
    assert any(n2 == TILE + 1 for n2 in n2s)                                # a last pass of one column
    assert any(WORDS * 32 < n2 <= TILE for n2 in n2s)                       # 17+ words per row, one pass
    assert any(WORDS * 32 < n2 <= TILE and n1 > ROUND_ROWS for n1, n2 in sizes)   # ... staged once, read in round two
    assert any(n2 <= WORDS * 32 and n1 > ROUND_ROWS for n1, n2 in sizes)    # preloaded words, two rounds
    assert any(n1 > ROUND_ROWS and (n1 - 1) // 64 % 4 != 3 for n1 in n1s)   # last round: some wavefronts have no rows
    assert any(n1 % 64 not in (0, 1) for n1 in n1s) and any(n1 % 64 == 1 for n1 in n1s)    # ragged last row block
    assert any(n2 % 4 != 0 for n2 in n2s) and any(n2 % 32 == 0 for n2 in n2s)             # scalar tail / none
    lengths = [e - b for _, n2 in sizes for b, e in quarters(n2)]
    assert any(n > ROWS_TILE for n in lengths) and any(n == 0 for n in lengths)
    assert any(n == ROWS_TILE + 1 for n in lengths)                         # a second tile of one column
    assert any(sum(e > b for b, e in quarters(n2)) == 1 for n2 in n2s)      # fewer words than quarters
    sel = rc.select()
    assert sel.shape == (3, len(sizes)) and sel[0].sum() == 0 and sel[1].sum() > SHARES and sel[2].sum() == 5
    assert all(sel[2, rc.PAIR_NAMES.index(p)] for p in rc.SUBSET_MUST)


def test_inadmissible_pairs_and_ties():
    masked, plain = rc.reference('grid', True), rc.reference('grid', False)
    empty = [p for p, name in enumerate(rc.PAIR_NAMES) if name in ((1, 'N0'), ('N0', 1), (1, 1))]
    for ref in (masked, rc.reference('raw', True)):
        assert (ref['flat'][:, empty] == -1).all() and (ref['ij'][:, empty] == -1).all() and (ref['min'][:, empty] == 0).all()
        rest = [p for p in range(len(rc.PAIR_NAMES)) if p not in empty]
        assert (ref['flat'][:, rest] >= 0).all()
    assert (plain['flat'] >= 0).all()
    # exact ties on the grid, the first index not the last
    tied = lambda ref: (ref['count'] > 1) & (ref['flat'] != ref['last'])
    assert tied(masked).any(0).sum() >= 3
    _, lists = rc.regions()
    for p, (ra, rb) in enumerate(rc.pairs()):
        if len(np.intersect1d(lists[ra], lists[rb])) >= 2:       # two shared vertices: d2 = 0 at least twice
            assert tied(plain)[:, p].all(), rc.PAIR_NAMES[p]
    # ... and once within ONE row and one column quarter of a body whose pairs are all selected (both kernels see it): only
    # the strict '<' of a lane's column loop decides that one
    p = rc.PAIR_NAMES.index((1602, 1602))
    n2 = rc.pair_sizes()[p][1]
    first = int(plain['flat'][1, p])
    cols = [first % n2, int(plain['row_last'][1, p]) % n2]
    assert rc.select()[1, p] and plain['row_last'][1, p] // n2 == first // n2 and cols[1] > cols[0]
    row = rc.pair_d2(rc.vertices('grid')[1], lists[rc.pairs()[p][0]][first // n2:first // n2 + 1], lists[rc.pairs()[p][1]])[0]
    b, e = quarters(n2)[0]
    zeros = np.flatnonzero(row[b:e] == 0.0) + b
    assert len(zeros) >= 2 and zeros[0] == cols[0] == 0 and zeros[1] < ROWS_TILE < e - b


def test_grid_d2_is_exact_in_float32():
    """The kernel's operation order in float32 (fma(dz, dz, fma(dy, dy, dx * dx)), all exact here) against float64."""
    names, lists = rc.regions()
    r1, r2 = lists[names.index(1100)], lists[names.index(520)]
    for b in range(3):
        v = rc.vertices('grid')[b]
        d = v[r1][:, None, :] - v[r2][None, :, :]
        assert d.dtype == np.float32
        d32 = d[..., 2] * d[..., 2] + (d[..., 1] * d[..., 1] + d[..., 0] * d[..., 0])
        assert d32.dtype == np.float32 and np.array_equal(d32.astype(np.float64), rc.pair_d2(v, r1, r2))


def test_gradient_reference_against_finite_differences():
    ref = rc.reference('raw', True)
    g = rc.upstream('raw')
    v = rc.vertices('raw').astype(np.float64)
    grad, s, n = rc.grad_reference(v, ref['ij'], g)
    assert (grad[s == 0] == 0).all() and (n[s > 0] > 0).all()

    def objective(x):
        total = 0.0
        for p in range(len(rc.PAIR_NAMES)):
            for b in range(3):
                i, j = ref['ij'][b, p]
                if i >= 0:
                    total += float(g[b, p]) * ((x[b, i] - x[b, j]) ** 2).sum()
        return total
    rng = np.random.default_rng(0)
    direction = rng.standard_normal(v.shape)
    h = 1e-6
    fd = (objective(v + h * direction) - objective(v - h * direction)) / (2 * h)
    assert abs(fd - (grad * direction).sum()) <= 1e-6 * np.abs(grad * direction).sum()
