"""What the caption-scoring feature can be held to without a GPU: the stored oracle outputs (tests/golden/captions_*.npz) are
what the project's oracle computes, the host-side planner of mjv_attention_ctx_bf16 lays every query out exactly once and
refuses bad shapes, and ``score_captions``' host checks name the offending row."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import captions_util as cu
from mj_video_amd import _lib, synth


def test_tiny_golden_is_the_oracle():
    """re-derives tests/golden/captions_tiny_one.npz (fp32 and bf16 oracle, twelve captions of one video) and compares bits"""
    f32, bf16 = cu.load_golden_captions("tiny", "one")
    for dtype, stored in ((torch.float32, f32), (torch.bfloat16, bf16)):
        now = cu.oracle_outputs("tiny", "one", dtype)
        for k in cu.ORACLE_FIELDS:
            assert now[k].shape == stored[k].shape and np.array_equal(now[k], stored[k]), (dtype, k)


@pytest.mark.parametrize("dims,case", [("tiny", "one"), ("tiny", "multi"), ("2b", "one"), ("2b", "multi")])
def test_golden_files_hold_every_field_per_caption(dims, case):
    f32, bf16 = cu.load_golden_captions(dims, case)
    assert os.path.getsize(cu.golden_path(dims, case)) < 1 << 20
    for stored in (f32, bf16):
        for k in cu.ORACLE_FIELDS:
            assert stored[k].shape[0] == 12 and np.isfinite(stored[k]).all(), (k, stored[k].shape)
    if case == "one":   # the order check of the GPU test is not vacuous: enough pairs lie 6 x the bf16 oracle's own noise apart
        s32, s16 = f32["score"], bf16["score"]
        thr = 6 * np.sqrt(np.mean((s16 - s32) ** 2))
        decisive = [(i, j) for i in range(12) for j in range(i + 1, 12) if abs(s32[i] - s32[j]) > thr]
        assert len(decisive) >= 24, len(decisive)
        assert all((s32[i] > s32[j]) == (s16[i] > s16[j]) for i, j in decisive)


@pytest.fixture(scope="module")
def lib():
    if not os.path.isfile(_lib.LIB_PATH):
        _lib.build_library()
    return _lib.load_library()


def plan_of(lib, cu_seq, index, cu_ctx, H=16, G=2, D=128, cu_q=None):
    arrs = [np.ascontiguousarray(np.asarray(a, dtype=np.int32)) for a in (cu_seq, index, cu_ctx)]
    q = None if cu_q is None else np.ascontiguousarray(np.asarray(cu_q, dtype=np.int32))
    d = _lib.AttnCtxDesc()
    d.cu_seqlens, d.context_index, d.cu_context = (a.ctypes.data for a in arrs)
    d.cu_seqlens_q = None if q is None else q.ctypes.data
    d.n_seqs, d.n_contexts, d.n_heads, d.kv_group, d.head_dim, d.causal = len(arrs[1]), len(arrs[2]) - 1, H, G, D, 1
    n = lib.mjv_attention_ctx_plan(C.byref(d), None, 0)
    if n < 0:
        return int(n), lib.mjv_last_error().decode(), None
    host = np.empty(n, dtype=np.int32)
    assert lib.mjv_attention_ctx_plan(C.byref(d), host.ctypes.data, n) == n
    assert lib.mjv_attention_ctx_plan(C.byref(d), host.ctypes.data, n - 1) == -1
    return int(n), int(lib.mjv_attention_ctx_workspace_bytes(C.byref(d))), host


def test_ctx_plan_places_every_query_once_and_cuts_contexts_by_their_own_shape(lib):
    """the planner runs on the host alone: every query row sits in exactly one stacked context tile and one own tile, a
    context's pieces cover its keys without gap or overlap, and a context's pieces do not move when another context joins"""
    G, TR = 2, 128
    QS = TR // G
    own = [1, 200, 75, 33, 160, 7]
    index = [0, 1, 0, 0, 1, 0]
    cu_seq = np.concatenate([[0], np.cumsum(own)])
    q_lens = [1, 5, 75, 2, 160, 7]
    cu_q = np.concatenate([[0], np.cumsum(q_lens)])
    n, ws, plan = plan_of(lib, cu_seq, index, [0, 2112, 2112 + 576], G=G, cu_q=cu_q)
    n_parts, n_tiles, total_q, g, n_kv = (int(x) for x in plan[1:6])
    assert total_q == sum(q_lens) and g == G and n_kv == 8
    assert ws == n_parts * n_kv * TR * (128 + 2) * 4
    parts = plan[8:8 + 4 * n_parts].reshape(-1, 4)
    tiles = plan[8 + 4 * n_parts:8 + 4 * n_parts + 8 * n_tiles].reshape(-1, 8)
    off = 8 + 4 * n_parts + 8 * n_tiles
    rowq = plan[off:off + n_tiles * QS].reshape(n_tiles, QS)
    qinfo = plan[off + 2 * n_tiles * QS:off + 2 * n_tiles * QS + 2 * total_q].reshape(total_q, 2)
    seen_ctx, seen_own = np.zeros(total_q, int), np.zeros(total_q, int)
    for t in range(n_tiles):
        kind, row0, nkeys, part0, nsplit, nrows = (int(x) for x in tiles[t, :6])
        assert nrows % G == 0 and 0 < nrows <= TR
        for j in range(nrows // G):
            (seen_own if kind else seen_ctx)[rowq[t, j]] += 1
            assert qinfo[rowq[t, j], kind] == t * QS + j
        ps = parts[part0:part0 + nsplit]
        assert (ps[:, 0] == t).all() and ps[0, 1] == 0 and (ps[1:, 1] == ps[:-1, 2]).all() and (ps[:, 1] % 64 == 0).all()
        if kind == 0:
            assert ps[-1, 2] == nkeys and nkeys in (2112, 576)
        else:
            assert nsplit == 1 and 0 < ps[0, 2] <= nkeys
    assert (seen_ctx == 1).all() and (seen_own == 1).all()
    # context 0 alone: same tiles, same cuts
    keep = [i for i, c in enumerate(index) if c == 0]
    _, _, alone = plan_of(lib, np.concatenate([[0], np.cumsum([own[i] for i in keep])]), [0] * len(keep), [0, 2112], G=G,
                          cu_q=np.concatenate([[0], np.cumsum([q_lens[i] for i in keep])]))
    a_parts = alone[8:8 + 4 * int(alone[1])].reshape(-1, 4)
    a_tiles = alone[8 + 4 * int(alone[1]):8 + 4 * int(alone[1]) + 8 * int(alone[2])].reshape(-1, 8)
    c0 = [t for t in range(n_tiles) if tiles[t, 0] == 0 and tiles[t, 1] == 0]
    a0 = [t for t in range(int(alone[2])) if a_tiles[t, 0] == 0]
    assert len(c0) == len(a0)
    for t, u in zip(c0, a0):
        assert tiles[t, 4] == a_tiles[u, 4] and tiles[t, 5] == a_tiles[u, 5]
        assert np.array_equal(parts[tiles[t, 3]:tiles[t, 3] + tiles[t, 4], 1:3], a_parts[a_tiles[u, 3]:a_tiles[u, 3] + a_tiles[u, 4], 1:3])


def test_ctx_plan_refusals(lib):
    for args, kw, code, text in [
        (([0, 5], [0], [0, 100]), {}, -1, "multiple of 64"),
        (([0, 5], [0], [0, 0]), {}, -1, "multiple of 64"),
        (([0, 5], [1], [0, 64]), {}, -1, "names context"),
        (([0, 5, 5], [0, 0], [0, 64]), {}, -1, "own rows"),
        (([0, 5], [0], [0, 64]), dict(cu_q=[0, 6]), -1, "queries"),
        (([0, 5], [0], [0, 64]), dict(D=64), -3, "head_dim 64"),
        (([0, 5], [0], [0, 64]), dict(D=96), -3, "head_dim 96"),
        (([0, 5], [0], [0, 64]), dict(H=6, G=3), -1, "kv_group"),
    ]:
        rc, msg, _ = plan_of(lib, *args, **kw)
        assert rc == code and text in msg, (args, kw, rc, msg)


def test_score_captions_host_checks_need_no_gpu():
    """``_analyse_captions`` is host code: every refusal names its row (the GPU test repeats them through the public call)"""
    from mj_video_amd.modeling import InternVLChatRewardModeling, VideoContext
    cfg, videos, prompts, index = cu.multi_case("tiny")
    model = InternVLChatRewardModeling.from_config(cfg, dtype=torch.bfloat16)
    model.config.pad_token_id = synth.PAD_ID
    model.model.img_context_token_id = synth.IMG_CONTEXT_ID
    ids, mask = synth.pad_batch(prompts)
    ids, mask = ids.numpy(), mask.numpy().astype(bool)
    ctxs = []
    for v in range(3):
        row = prompts[int(np.flatnonzero(index == v)[0])][0].numpy()
        cols = np.flatnonzero(row == synth.IMG_CONTEXT_ID)
        P = (int(cols[-1]) + 1) // 64 * 64
        ctxs.append(VideoContext(row[:P].copy(), P, [], [], torch.empty(int((cols >= P).sum()), 8), cols[cols >= P], cols.size, None,
                                 None, None, torch.device("cpu")))
    info = model._analyse_captions(ids, mask, ctxs, index, group=False)
    assert info["total"] == int(mask.sum()) - sum(ctxs[int(c)].P for c in index)
    assert (np.diff(info["cu"]) == mask.sum(1) - np.array([ctxs[int(c)].P for c in index])).all()
    assert (info["index"] == index).all() and (info["img_src"] >= 0).sum() == sum(ctxs[int(c)].tail_cols.size for c in index)
    grouped = model._analyse_captions(ids, mask, ctxs, index, group=True)
    assert (np.diff(grouped["index"]) >= 0).all() and grouped["total"] == info["total"]
    # the selected rows follow the ORIGINAL row order whatever the packing order: same tokens under both
    assert (grouped["ids"][grouped["sel_rows"]] == info["ids"][info["sel_rows"]]).all()
    bad = ids.copy()
    bad[7, 3] += 1
    with pytest.raises(ValueError, match="row 7: its first"):
        model._analyse_captions(bad, mask, ctxs, index, group=False)
    m2 = mask.copy()
    m2[9, 10] = False
    with pytest.raises(ValueError, match="row 9: masked column 10"):
        model._analyse_captions(ids, m2, ctxs, index, group=False)
    with pytest.raises(ValueError, match=r"row 0: \d+ <IMG_CONTEXT> tokens"):
        model._analyse_captions(ids, mask, ctxs, np.roll(index, 1), group=False)
