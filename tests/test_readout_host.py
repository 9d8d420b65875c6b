"""The frame readout (mjv_attention_readout_bf16, include/mjv.h; model.frame_readout) as far as a CPU can hold it: the plan builder
through the library (sizes, contents, every refusal with its code and a word of its message), layout.readout_bins on hand-written
ids, the binding's symbols, and the model's switch on the host constructor path."""
import ctypes as C

import numpy as np
import pytest
import torch

import mj_video_amd  # noqa: F401
from mj_video_amd import _lib, layout, ops

CTX, PAD = 9, 0
PATTERN = (7, 8)
RULES = layout.TokenRules(pad_id=PAD, ctx_id=CTX, vocab=100, tokens_per_tile=2, gating_pattern=PATTERN)


# ------------------------------------------------------------------------------------------------ the plan
def make_plan(ranges, edges, head_dim=128, mode=2, n_tensors=None, H=4, G=2):
    return ops.AttnReadoutPlan(ranges, edges, H, G, head_dim, mode, device=None, n_tensors=n_tensors)


def test_plan_sizes_and_contents():
    """header, query table, range table (with every range's first key position) and edges: the int32 image of the host arrays"""
    ranges = [[(0, 0, 64), (1, 10, 7)], [(1, 3, 5)], [(0, 0, 64), (1, 20, 1), (2, 0, 9)]]
    edges = [[0, 64, 70, 71], [0, 5], [0, 1, 1, 64, 74]]
    p = make_plan(ranges, edges)
    nq, nr, ne = 3, 6, 4 + 2 + 5
    assert p.plan_ints == p.host.size == 8 + 4 * nq + 4 * nr + ne
    assert p.max_bins == 4 and p.n_tensors == 3 and p.n_queries == 3
    h = p.host
    off_r, off_e = 8 + 4 * nq, 8 + 4 * nq + 4 * nr
    assert h[1:7].tolist() == [nq, nr, ne, off_r, off_e, p.plan_ints] and h[7] == 0
    assert h[8:8 + 4 * nq].reshape(nq, 4).tolist() == [[0, 2, 0, 3], [2, 1, 4, 1], [3, 3, 6, 4]]
    assert h[off_r:off_e].reshape(nr, 4).tolist() == [[0, 0, 64, 0], [1, 10, 7, 64], [1, 3, 5, 0], [0, 0, 64, 0], [1, 20, 1, 64], [2, 0, 9, 65]]
    assert h[off_e:].tolist() == [e for qe in edges for e in qe]
    # head_dim 96 and mode 1 plan alike: the plan depends on the index arrays alone
    assert np.array_equal(make_plan(ranges, edges, head_dim=96, mode=1).host, h)
    # a short buffer is refused, not overrun
    d = p.desc()
    small = np.zeros(4, dtype=np.int32)
    assert _lib.load_library().mjv_attention_readout_plan(C.byref(d), small.ctypes.data, 4) == -1
    assert not small.any()


@pytest.mark.parametrize("kw,code,word", [
    (dict(head_dim=64), -3, "head_dim 64"),
    (dict(mode=0), -1, "score_round_mode 0"),
    (dict(edges=[[0]]), -1, "0 bins"),
    (dict(edges=[list(range(129)) + [300]], ranges=[[(0, 0, 300)]]), -1, "129 bins"),
    (dict(edges=[[0, 40, 30, 71]]), -1, "not ascending"),
    (dict(edges=[[0, 40, 70]]), -1, "last bin edge 70"),
    (dict(edges=[[5, 40, 71]]), -1, "first bin edge 5"),
    (dict(ranges=[[(0, 0, 71), (1, 4, 0)]]), -1, "range 1"),
    (dict(ranges=[[(0, 0, 64), (2, 0, 7)]], n_tensors=2), -1, "range_tensor 2"),
    (dict(ranges=[[(0, 0, 64), (-1, 0, 7)]], n_tensors=2), -1, "range_tensor -1"),
    (dict(ranges=[[]], edges=[[0, 71]]), -1, "query 0 has no key range"),
    (dict(H=4, G=3), -1, "kv_group 3"),
])
def test_plan_refusals(kw, code, word):
    args = dict(ranges=[[(0, 0, 64), (1, 10, 7)]], edges=[[0, 64, 71]], n_tensors=2)
    args.update(kw)
    with pytest.raises(_lib.MjvLibraryError) as e:
        make_plan(**args)
    assert f"({code})" in str(e.value) and word in str(e.value), str(e.value)


def test_plan_refusal_names_the_query():
    with pytest.raises(_lib.MjvLibraryError, match="query 1"):
        make_plan([[(0, 0, 5)], [(0, 0, 5)]], [[0, 5], [0, 4]])
    assert make_plan([[(0, 0, 300)]], [list(range(128)) + [300]]).max_bins == 128      # 128 bins are taken
    assert make_plan([[(0, 0, 1)]], [[0, 1]]).plan_ints == 8 + 4 + 4 + 2               # one key, one bin


def test_symbols_and_abi():
    for name in ("mjv_attention_readout_plan", "mjv_attention_readout_bf16"):
        assert name in _lib.SYMBOLS and hasattr(_lib.load_library(), name)
    assert issubclass(_lib.AttnReadoutDesc, C.Structure)      # mjv_attn_readout_desc
    assert _lib.ABI_VERSION == 7 and _lib.load_library().mjv_abi_version() == 7


# ------------------------------------------------------------------------------------------------ layout.readout_bins
def prompt(frames, caption=3, labels=True, before_last=None):
    """hand-written ids: 2 system tokens, per frame (a label when ``labels``) + its image tokens, caption tokens, the gating
    pattern; text ids 20 .."""
    ids, t = [20, 21], 30
    for f, n in enumerate(frames):
        if labels:
            ids.append(t)
            t += 1
        ids += [CTX] * n
    ids += list(range(50, 50 + caption)) + list(PATTERN)
    return np.asarray(ids)


def test_bins_interleaved_labels_against_one_long_run():
    a = layout.readout_bins(RULES, prompt([2, 2, 2]), np.arange(16), 1)
    # sys sys L0 I I L1 I I L2 I I c c c g g : text, frame 0, text, frame 1, text, frame 2, caption
    assert a.n_frames == 3
    assert a.reward.keys == 16 and a.reward.edges.tolist() == [0, 3, 5, 6, 8, 9, 11, 16] and a.reward.fold.tolist() == [3, 0, 3, 1, 3, 2, 4]
    assert a.gating.keys == 15 and a.gating.edges.tolist() == [0, 3, 5, 6, 8, 9, 11, 15] and a.gating.fold.tolist() == [3, 0, 3, 1, 3, 2, 4]
    b = layout.readout_bins(RULES, prompt([2, 2, 2], labels=False), np.arange(13), 1)
    # sys sys I I I I I I c c c g g : text, frame 0, frame 1, frame 2, caption - no empty text bins
    assert b.reward.edges.tolist() == [0, 2, 4, 6, 8, 13] and b.reward.fold.tolist() == [3, 0, 1, 2, 4]
    assert b.gating.keys == 12 and b.gating.edges[-1] == 12
    assert b.reward.edges.dtype == np.int32 and b.reward.fold.dtype == np.int32


def test_bins_tiles_per_frame():
    ids = prompt([2, 2, 4])               # three runs of 1, 1, 2 tiles
    one = layout.readout_bins(RULES, ids, np.arange(ids.size), 1)
    assert one.n_frames == 4              # the long run is dealt to two frames: it splits into two bins
    assert one.reward.fold.tolist() == [4, 0, 4, 1, 4, 2, 3, 5]
    lst = layout.readout_bins(RULES, ids, np.arange(ids.size), [2, 1, 1])
    assert lst.n_frames == 3              # frame 0 = the first two runs: two bins with the label between them, one column
    assert lst.reward.fold.tolist() == [3, 0, 3, 0, 3, 1, 2, 4]
    assert lst.reward.edges.tolist() == one.reward.edges.tolist()
    two = layout.readout_bins(RULES, ids, np.arange(ids.size), 2)
    assert two.n_frames == 2 and two.reward.fold.tolist() == [2, 0, 2, 0, 2, 1, 3]
    for bad in (3, [2, 1], [1, 1, 1, 2], [4, 0], 0):
        with pytest.raises(ValueError, match="tiles_per_frame"):
            layout.readout_bins(RULES, ids, np.arange(ids.size), bad)


def test_bins_padding_and_holes():
    ids = prompt([2, 2])
    n = ids.size                                       # 13: sys sys L I I L I I c c c g g
    ref = layout.readout_bins(RULES, ids, np.arange(n), 1)
    right = np.concatenate([ids, [PAD] * 4])
    r = layout.readout_bins(RULES, right, np.arange(n), 1)
    assert r.reward.keys == ref.reward.keys == n and r.reward.edges.tolist() == ref.reward.edges.tolist()
    left = np.concatenate([[PAD] * 4, ids])            # valid tokens at the end: packed key i = column 4 + i
    # (the reward column of a row that STARTS with the pad id is its last column: layout.selected_columns)
    lft = layout.readout_bins(RULES, left, 4 + np.arange(n), 1)
    assert lft.reward.keys == n and lft.reward.edges.tolist() == ref.reward.edges.tolist() and lft.gating.keys == ref.gating.keys
    # holes: the first label and one caption token masked out - packed coordinates close up
    cols = np.asarray([c for c in range(n) if c not in (2, 9)])
    h = layout.readout_bins(RULES, ids, cols, 1)
    # sys sys [L] I I L I I c [c] c g g -> text(2) frame0(2) text(1) frame1(2) caption(4)
    assert h.reward.keys == n - 2 and h.reward.edges.tolist() == [0, 2, 4, 5, 7, 11] and h.reward.fold.tolist() == [2, 0, 2, 1, 3]
    with pytest.raises(ValueError, match="IMG_CONTEXT"):
        layout.readout_bins(RULES, ids, np.asarray([c for c in range(n) if c != 3]), 1)
    with pytest.raises(ValueError, match="gating row"):
        layout.readout_bins(RULES, ids, np.asarray([c for c in range(n) if c != n - 2]), 1)


def test_bins_of_a_row_before_the_last_frame():
    """a gating pattern in front of the last frame: the gating row sees frame 0 whole, nothing of frame 1; a reward row inside the
    last frame (the row ends there: pad follows) sees a partial bin"""
    ids = np.asarray([20, 30, CTX, CTX, 7, 8, 31, CTX, CTX, 50, 51])
    b = layout.readout_bins(RULES, ids, np.arange(ids.size), 1)
    assert b.gating.keys == 5 and b.gating.edges.tolist() == [0, 2, 4, 5] and b.gating.fold.tolist() == [2, 0, 2]
    assert b.reward.keys == 11 and b.reward.fold.tolist() == [2, 0, 2, 1, 3]
    cut = np.concatenate([ids[:8], [PAD] * 3])        # the last valid token is the first image token of frame 1
    with pytest.raises(ValueError, match="tiles_per_frame"):      # (one image token less: the count no longer fits)
        layout.readout_bins(RULES, cut, np.arange(8), 1)
    rules1 = RULES._replace(tokens_per_tile=1)
    c = layout.readout_bins(rules1, cut, np.arange(8), [2, 1])
    assert c.reward.keys == 8 and c.reward.edges.tolist() == [0, 2, 4, 7, 8] and c.reward.fold.tolist() == [2, 0, 2, 1]
    d = layout.readout_bins(rules1, cut, np.arange(8), [1, 2])     # frame 1 = tokens 3 and 7: the row sees half of it
    assert d.reward.edges.tolist() == [0, 2, 3, 4, 7, 8] and d.reward.fold.tolist() == [2, 0, 1, 2, 1]


def test_bins_feed_the_plan():
    """the edges of readout_bins are what mjv_attention_readout_plan takes: first 0, ascending, last = the key count"""
    ids = prompt([2, 2, 4])
    b = layout.readout_bins(RULES, ids, np.arange(ids.size), [2, 1, 1])
    p = make_plan([[(0, 0, b.reward.keys)], [(0, 0, b.gating.keys)]], [b.reward.edges, b.gating.edges])
    assert p.max_bins == b.reward.fold.size


# ------------------------------------------------------------------------------------------------ the model's switch
def test_model_default_is_off():
    from mj_video_amd import configuration as cfgs
    from mj_video_amd.modeling import FrameReadout, InternVLChatRewardModeling
    import copy
    cfg = cfgs.InternVLChatRewardModelingConfig(**copy.deepcopy(cfgs.tiny_config_dict(56)), **cfgs.mjvideo_head_kwargs())
    model = InternVLChatRewardModeling.from_config(cfg, dtype=torch.bfloat16)
    assert model.frame_readout is False and model.last_readout is None and model.readout_tiles_per_frame == 1
    mass = torch.arange(2 * 2 * 3 * 2 * 5, dtype=torch.float32).view(2, 2, 3, 2, 5)
    ro = FrameReadout(mass, np.asarray([3, 2]))
    assert ro.per_frame().shape == (2, 3) and torch.equal(ro.per_frame(), mass[:, 0, :, :, :3].mean(dim=(1, 2)))
    assert torch.equal(ro.per_frame("gating", layers=[2]), mass[:, 1, 2, :, :3].mean(dim=1))
    with pytest.raises(ValueError):
        ro.per_frame("other")
