"""CPU checks of the draft-tree helpers (gear_amd/speculative.py): tree_layout against a walk up the parents, tree_accept against
a plain Python walk (sibling tokens collide on purpose), ngram_tree_draft (width 1 = ngram_draft, both continuations of a repeated
n-gram present, always a valid tree)."""
import pytest
import torch

from gear_amd.speculative import accepted_lengths, ngram_draft, ngram_tree_draft, tree_accept, tree_layout

CHAIN7 = [-1, 0, 1, 2, 3, 4, 5]
STAR7 = [-1, 0, 0, 0, 0, 0, 0]
BINARY7 = [-1, 0, 0, 1, 1, 2, 2]
TWO_CHAINS16 = [-1, 0, 0] + list(range(1, 14))            # 1-3-5-..-15 and 2-4-6-..-14 under the root


def _walk_up(par, i):
    mask = depth = 0
    while i >= 0:
        mask |= 1 << i
        i = par[i]
        depth += 1
    return mask, depth - 1


def _masks(anc):
    return [int(x) & 0xFFFFFFFF for x in anc.view(torch.int32).reshape(-1).tolist()]


@pytest.mark.parametrize("par", [CHAIN7, STAR7, BINARY7, TWO_CHAINS16, list(range(-1, 15)), [-1]],
                         ids=["chain", "star", "binary7", "two-chains16", "chain16", "root-only"])
def test_tree_layout_matches_a_walk_up_the_parents(par):
    n = len(par)
    anc, depth = tree_layout(torch.tensor(par))
    assert anc.dtype == torch.uint32 and depth.dtype == torch.long and anc.shape == depth.shape == (1, n)
    want = [_walk_up(par, i) for i in range(n)]
    assert _masks(anc) == [w[0] for w in want]
    assert depth[0].tolist() == [w[1] for w in want]
    if par == list(range(-1, n - 1)):
        assert _masks(anc) == [(2 << i) - 1 for i in range(n)]
        assert depth[0].tolist() == list(range(n))


def test_tree_layout_batched_and_random():
    g = torch.Generator().manual_seed(0)
    for n in (2, 5, 16):
        par = torch.stack([torch.cat([torch.tensor([-1])] + [torch.randint(0, i, (1,), generator=g) for i in range(1, n)])
                           for _ in range(6)])
        anc, depth = tree_layout(par)
        assert anc.shape == depth.shape == (6, n)
        for b in range(6):
            want = [_walk_up(par[b].tolist(), i) for i in range(n)]
            assert _masks(anc[b]) == [w[0] for w in want] and depth[b].tolist() == [w[1] for w in want]


def test_tree_layout_refusals():
    with pytest.raises(ValueError):
        tree_layout(torch.tensor(list(range(-1, 16))))                 # n = 17
    with pytest.raises(ValueError):
        tree_layout(torch.tensor([0, 0, 1]))                           # parents[0] != -1
    with pytest.raises(ValueError):
        tree_layout(torch.tensor([-1, 0, 2]))                          # a node its own parent
    with pytest.raises(ValueError):
        tree_layout(torch.tensor([-1, 2, 0]))                          # a parent after its node
    with pytest.raises(ValueError):
        tree_layout(torch.tensor([-1, -1, 0]))                         # a second root
    with pytest.raises(ValueError):
        tree_layout(torch.tensor([[-1, 0, 1], [-1, 0, 2]]))            # one bad row of a batch


def _accept_walk(tok, par, logits):
    n = len(tok)
    u, path = 0, [0]
    while True:
        t = int(logits[u].argmax())
        kids = [c for c in range(n) if par[c] == u and tok[c] == t]
        if not kids:
            return path, t
        u = kids[0]
        path.append(u)


def test_tree_accept_matches_a_python_walk():
    g = torch.Generator().manual_seed(1)
    V, B = 3, 8                                                        # 3 tokens: siblings collide, paths run deep
    duplicates = deep = 0
    for n in (1, 2, 7, 16):
        for _ in range(12):
            par = torch.stack([torch.cat([torch.tensor([-1])] + [torch.randint(max(0, i - 3), i, (1,), generator=g)
                                                                 for i in range(1, n)]) for _ in range(B)])
            tok = torch.randint(0, V, (B, n), generator=g)
            logits = torch.randn(B, n, V, generator=g)
            path, length, nxt = tree_accept(tok, par, logits)
            assert path.shape == (B, n) and length.shape == nxt.shape == (B,)
            for b in range(B):
                want, t = _accept_walk(tok[b].tolist(), par[b].tolist(), logits[b])
                assert path[b].tolist() == want + [-1] * (n - len(want)), (n, b)
                assert int(length[b]) == len(want) and int(nxt[b]) == t
                deep += len(want) >= 3
                p, tk = par[b].tolist(), tok[b].tolist()          # a later sibling with the token of a node on the path
                duplicates += any(p[c] == p[d] and tk[c] == tk[d] for c in want[1:] for d in range(c + 1, n))
    assert duplicates > 10 and deep > 10                               # the duplicate-child rule was exercised


def test_tree_accept_shared_parents_and_chain_equals_accepted_lengths():
    g = torch.Generator().manual_seed(2)
    B, k, V = 6, 7, 4
    drafts = torch.randint(0, V, (B, k), generator=g)
    logits = torch.randn(B, k + 1, V, generator=g)
    logits[0, torch.arange(k), drafts[0]] += 10.0                      # row 0 accepts everything
    logits[1, torch.arange(3), drafts[1, :3]] += 10.0                  # row 1 at least three
    tok = torch.cat([torch.zeros(B, 1, dtype=torch.long), drafts], 1)
    chain = torch.arange(-1, k)                                        # [n]: one tree for every row
    path, length, nxt = tree_accept(tok, chain, logits)
    want = accepted_lengths(drafts, logits)
    assert torch.equal(length - 1, want) and int(want[0]) == k and int(want[1]) >= 3
    for b in range(B):
        a = int(want[b])
        assert path[b].tolist() == list(range(a + 1)) + [-1] * (k - a)
        assert int(nxt[b]) == int(logits[b, a].argmax())


def test_ngram_tree_draft_width_one_is_ngram_draft():
    g = torch.Generator().manual_seed(3)
    for L in (1, 2, 5, 40):
        toks = torch.randint(0, 4, (5, L), generator=g)
        for n_nodes in (1, 2, 5, 16):
            for mx in (1, 3):
                d, par = ngram_tree_draft(toks, n_nodes, width=1, max_ngram=mx)
                assert torch.equal(d, ngram_draft(toks, n_nodes - 1, mx))
                assert torch.equal(par, torch.arange(-1, n_nodes - 1).expand(5, n_nodes))


def _branches(d, par):
    """Every root-to-leaf token sequence of one row's tree."""
    n = len(par)
    tok = [None] + d
    leaves = [i for i in range(1, n) if i not in par]
    out = []
    for leaf in leaves:
        seq, i = [], leaf
        while i > 0:
            seq.append(tok[i])
            i = par[i]
        out.append(seq[::-1])
    return out


def test_ngram_tree_draft_keeps_both_continuations():
    #            0  1  2   3   4   5  6  7   8   9  10  11 12
    row = [[9, 1, 2, 30, 31, 32, 7, 1, 2, 40, 41, 42, 8, 1, 2]]       # the bigram (1, 2) twice before, two continuations
    d, par = ngram_tree_draft(torch.tensor(row), 8, width=2, max_ngram=2)
    assert d.shape == (1, 7) and par.shape == (1, 8)
    tree_layout(par)
    br = _branches(d[0].tolist(), par[0].tolist())
    assert sorted(br) == [[30, 31, 32], [40, 41, 42, 8]]               # 7 nodes: 4 for the most recent occurrence, 3 for the other
    assert d[0].tolist()[:4] == [40, 41, 42, 8]                        # the most recent occurrence comes first
    # a shared first token is one node
    row = [[1, 2, 5, 60, 7, 1, 2, 5, 61, 8, 1, 2]]
    d, par = ngram_tree_draft(torch.tensor(row), 7, width=2, max_ngram=2)
    br = _branches(d[0].tolist(), par[0].tolist())
    assert sorted(b[:2] for b in br) == [[5, 60], [5, 61]] and d[0].tolist().count(5) == 1
    # width 2 with one occurrence only: the chain of ngram_draft
    row = torch.tensor([[3, 4, 5, 6, 3, 4]])
    d, par = ngram_tree_draft(row, 6, width=2)
    assert torch.equal(d, ngram_draft(row, 5)) and par[0].tolist() == [-1, 0, 1, 2, 3, 4]


def test_ngram_tree_draft_is_always_a_valid_tree():
    g = torch.Generator().manual_seed(4)
    for L in (1, 3, 12, 60):
        for vocab in (2, 3, 8):
            toks = torch.randint(0, vocab, (6, L), generator=g)
            for n_nodes in (1, 2, 3, 8, 16):
                for width in (1, 2, 3, 5):
                    d, par = ngram_tree_draft(toks, n_nodes, width=width)
                    assert d.shape == (6, n_nodes - 1) and par.shape == (6, n_nodes)
                    assert d.dtype == par.dtype == torch.long
                    anc, depth = tree_layout(par)
                    assert anc.shape == (6, n_nodes)
                    for b in range(6):                                 # a trie: no two children of a node carry one token
                        seen = set()
                        for i in range(1, n_nodes):
                            key = (int(par[b, i]), int(d[b, i - 1]))
                            assert key not in seen
                            seen.add(key)
    with pytest.raises(ValueError):
        ngram_tree_draft(torch.zeros(1, 4, dtype=torch.long), 17)
    with pytest.raises(ValueError):
        ngram_tree_draft(torch.zeros(1, 4, dtype=torch.long), 0)
