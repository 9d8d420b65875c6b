"""The token-layout rules of ``mj_video_amd.layout``, each where it lives: pure numpy, no model (but for the one test that holds a
model's delegate to the function it calls)."""
import numpy as np
import pytest

from mj_video_amd import harness, layout, synth

PAD = synth.PAD_ID
GP = list(synth.GATING_PATTERN)
RULES = layout.TokenRules(pad_id=PAD, ctx_id=synth.IMG_CONTEXT_ID, vocab=92553, tokens_per_tile=4, gating_pattern=None)

# hand-written rows -> (pad_id, r, g)
TEXT = [1, 1500, 1501, 1502, 1503, 1504, 1505]
ROWS = {
    "pad_id None": (np.array(TEXT + GP + [PAD, PAD]), None, 13, 7),
    "no pad in the row": (np.array(TEXT + GP), PAD, 11, 7),
    "right-padded": (np.array(TEXT + GP + [PAD, PAD, PAD]), PAD, 11, 7),
    "pad at column 0": (np.array([PAD, PAD] + TEXT + GP), PAD, 13, 9),            # (0 - 1) % N wraps to N - 1
    "two patterns": (np.array(TEXT[:3] + GP + TEXT[3:] + GP + [PAD]), PAD, 16, 12),   # the last one wins
}


def test_layout_imports_numpy_alone():
    import ast
    tree = ast.parse(open(layout.__file__).read())
    names = {a.name for n in ast.walk(tree) if isinstance(n, ast.Import) for a in n.names}
    names |= {("." * n.level) + (n.module or "") for n in ast.walk(tree) if isinstance(n, ast.ImportFrom)}
    assert names == {"__future__", "typing", "numpy"}, names


@pytest.mark.parametrize("name", list(ROWS))
def test_selected_columns(name):
    row, pad_id, r, g = ROWS[name]
    assert layout.selected_columns(row, pad_id) == (r, g)
    assert layout.selected_columns(row, pad_id, GP[1:3]) == (r, g + 1), "another tokenizer's marker: its own last occurrence"


def test_selected_columns_without_a_pattern():
    with pytest.raises(ValueError, match="Token pattern not found in the list."):
        layout.selected_columns(np.array(TEXT + GP[:4] + [PAD]), PAD)
    with pytest.raises(ValueError, match="Token pattern not found in the list."):
        layout.selected_columns(np.array(GP[:3]), None)


def test_shared_prefix_len_is_the_selected_columns_under_the_common_prefix():
    for name, (row, pad_id, r, g) in ROWS.items():
        assert harness.shared_prefix_len([row], pad_id) == min(r, g), name
        assert harness.shared_prefix_len([row, row.copy()], pad_id) == min(r, g), name
        for cut in (1, 3, min(r, g), min(r, g) + 1, row.shape[0] - 1):      # a second row that leaves the first at column ``cut``
            other = row.copy()
            other[cut] += 1 if other[cut] != PAD else 7
            try:
                ro, go = layout.selected_columns(other, pad_id)
            except ValueError:
                continue            # (the edit broke the only pattern)
            assert harness.shared_prefix_len([row, other], pad_id) == min(cut, r, g, ro, go), (name, cut)
    a, b = ROWS["no pad in the row"][0], ROWS["two patterns"][0]           # rows of different lengths: the first three ids agree
    assert harness.shared_prefix_len([a, b], PAD) == 3
    with pytest.raises(ValueError, match="Token pattern not found"):
        harness.shared_prefix_len([np.array(TEXT)], PAD)


@pytest.mark.parametrize("r_first", [True, False])
def test_pack_tails(r_first):
    """three sequences of 5, 1 and 9 tokens, packed one behind the other, positions with holes; the selected rows in both orders"""
    lengths = (5, 1, 9)
    sel = [(1, 3), (0, 0), (4, 8)]                   # (lower, upper) index of the two selected tokens of each sequence
    rng = np.random.default_rng(5)
    ids = rng.integers(1000, 2000, size=sum(lengths))
    seqs, base = [], 0
    for L, (lo, hi) in zip(lengths, sel):
        cols = np.cumsum(rng.integers(1, 4, size=L))              # ascending columns, some skipped
        lr, lg = (lo, hi) if r_first else (hi, lo)
        seqs.append((base, lr, lg, L, cols))
        base += L
    tail_rows, tail_pos, cu_tail, sel_r, sel_g = layout.pack_tails(seqs)
    want_rows, want_pos, want_cu, want_r, want_g = [], [], [0], [], []
    for base, lr, lg, L, cols in seqs:                            # the plain loop: every token from the first selected one on
        first = min(lr, lg)
        for i in range(first, L):
            if i == lr:
                want_r.append(len(want_rows))
            if i == lg:
                want_g.append(len(want_rows))
            want_rows.append(base + i)
            want_pos.append(int(cols[i]))
        want_cu.append(len(want_rows))
    assert tail_rows.tolist() == want_rows and tail_pos.tolist() == want_pos and cu_tail.tolist() == want_cu
    assert [int(x) for x in sel_r] == want_r and [int(x) for x in sel_g] == want_g
    assert all(a.dtype == np.int32 for a in (tail_rows, tail_pos, cu_tail))
    sel_in_tail = np.asarray(list(sel_r) + list(sel_g))
    selected = [s[0] + s[1] for s in seqs] + [s[0] + s[2] for s in seqs]
    assert np.array_equal(ids[tail_rows[sel_in_tail]], ids[selected])
    assert np.diff(cu_tail).tolist() == [4, 1, 5]


def test_context_length():
    N = 200
    for last in (0, 62, 63, 64, 100, 127, 128, 198):
        cols = np.arange(max(0, last - 7), last + 1)
        assert layout.context_length(cols, N, None) == (last + 1) // 64 * 64
    assert layout.context_length(np.arange(0), N, None) == 0
    cols = np.arange(71, 103)
    for k in range(1, N):
        assert layout.context_length(cols, N, k) == k
        assert layout.context_length(cols, N, np.int64(k)) == k and type(layout.context_length(cols, N, np.int64(k))) is int
    for bad in (0, N, -1, True, 64.0, "64"):
        with pytest.raises(ValueError, match=rf"video 3: context_len must be None or an int in \[1, {N - 1}\]"):
            layout.context_length(cols, N, bad, "video 3: ")


def test_the_small_rules_refuse_what_they_name():
    assert layout.normalise_mask(None, (2, 3)).all() and layout.normalise_mask(np.array([[1, 0, 2]]), (1, 3)).tolist() == [[True, False, True]]
    with pytest.raises(ValueError, match=r"attention_mask shape \(1, 2\) != input_ids shape \(1, 3\)"):
        layout.normalise_mask(np.ones((1, 2)), (1, 3))
    layout.check_vocabulary(np.array([0, 92552]), 92553)
    layout.check_vocabulary(np.arange(0), 92553)
    for bad in (-1, 92553):
        with pytest.raises(IndexError, match=rf"video 1: token id out of range \[0, 92553\): min {min(bad, 5)}, max {max(bad, 5)}"):
            layout.check_vocabulary(np.array([5, bad]), 92553, "video 1: ")
    row = np.arange(6)
    assert layout.one_prompt(row, "ONE prompt") is row and np.array_equal(layout.one_prompt(row[None], "ONE prompt"), row)
    with pytest.raises(ValueError, match=r"ONE prompt per video \(\[N\] or \[1, N\]\), got input_ids of shape \(2, 3\)"):
        layout.one_prompt(row.reshape(2, 3), "ONE prompt per video")
    assert layout.check_pixels(((3, 3, 56, 56), "torch.bfloat16")) == 3
    with pytest.raises(ValueError, match="wrong pixel_values size"):
        layout.check_pixels(((3, 56, 56), "torch.bfloat16"))
    with pytest.raises(TypeError, match=r"must be bfloat16 like the model \(got torch.float32\)"):
        layout.check_pixels(((3, 3, 56, 56), "torch.float32"))
    am = np.ones(10, dtype=np.int64)
    am[6] = 0
    layout.check_context_unmasked(None, 10, 9)
    layout.check_context_unmasked(am[None], 10, 6)
    with pytest.raises(ValueError, match=r"masked column 6 inside the context \(7 tokens\)"):
        layout.check_context_unmasked(am, 10, 7)
    with pytest.raises(ValueError, match="attention_mask of 10 columns, the prompt has 11"):
        layout.check_context_unmasked(am, 11, 3)


def test_the_model_method_is_a_delegate():
    """one batch with a holey mask: ``layout.analyse_ids`` called directly and through the model, key for key"""
    import torch
    from mj_video_amd.chat_input import num_image_tokens_per_tile
    from mj_video_amd.modeling import InternVLChatRewardModeling
    from util import make_cfg
    cfg = make_cfg("tiny", 56)
    per = num_image_tokens_per_tile(cfg)
    model = InternVLChatRewardModeling.from_config(cfg, dtype=torch.bfloat16)
    model.config.pad_token_id = PAD
    model.model.img_context_token_id = synth.IMG_CONTEXT_ID
    ids, mask = synth.pad_batch([synth.synth_input_ids(t * per, 40 + t) for t in (4, 2, 3)])
    ids, mask = synth.remask(ids, mask, "holes")
    ids, mask = ids.numpy(), mask.numpy().astype(bool)
    rules = RULES._replace(tokens_per_tile=per, gating_pattern=tuple(GP))     # (the config names the reference's pattern)
    assert model._token_rules() == rules
    for lookup in (None, lambda p: True):
        direct = layout.analyse_ids(rules, ids, mask, 9, lookup)
        through = model._analyse_ids(ids, mask, 9, lookup)
        assert list(direct) == list(through)
        for k, v in direct.items():
            w = through[k]
            if isinstance(v, np.ndarray):
                assert w.dtype == v.dtype and np.array_equal(v, w), k
            else:
                assert type(v) is type(w) and v == w, k
        assert direct["skip"] == (64 if lookup else 0) and direct["total"] == int(mask.sum()) - 3 * direct["skip"]
