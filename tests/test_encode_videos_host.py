"""What ``encode_videos`` and the per-context addressing of mjv_attention_ctx_bf16 can be held to without a GPU: the planner
writes every context tile's context number and moves nothing else, a fresh descriptor names no pointer lists, the host checks
of ``encode_videos`` name the video, and ``ops.attention_ctx`` refuses a bad context tensor before anything is launched."""
import ctypes as C

import numpy as np
import pytest
import torch

import captions_util as cu
from mj_video_amd import _lib, ops, synth
from test_captions_host import lib, plan_of  # noqa: F401  (``lib``: the module's library fixture)

BF = torch.bfloat16
D = 128


def split_plan(plan):
    n_parts, n_tiles = int(plan[1]), int(plan[2])
    parts = plan[8:8 + 4 * n_parts].reshape(-1, 4)
    tiles = plan[8 + 4 * n_parts:8 + 4 * n_parts + 8 * n_tiles].reshape(-1, 8)
    return parts, tiles, plan[8 + 4 * n_parts + 8 * n_tiles:]


def test_plan_carries_the_context_number_and_nothing_else_moves(lib):  # noqa: F811
    """te[6] of a context tile = its context's number (own tiles: 0), also where a context has no sequence or the contexts are
    named out of order; every other plan field of the shapes of test_captions_host.py is what it was: recomputed here from the
    layout rules that test states (the first K / V row is still the context's cu_context row)."""
    own = [1, 200, 75, 33, 160, 7]
    index = [0, 1, 0, 0, 1, 0]
    q_lens = [1, 5, 75, 2, 160, 7]
    cu_seq, cu_q = np.concatenate([[0], np.cumsum(own)]), np.concatenate([[0], np.cumsum(q_lens)])
    cu_ctx = [0, 2112, 2112 + 576]
    n, ws, plan = plan_of(lib, cu_seq, index, cu_ctx, G=2, cu_q=cu_q)
    parts, tiles, _ = split_plan(plan)
    row0_to_ctx = {0: 0, 2112: 1}
    n_ctx_tiles = 0
    for te in tiles:
        if te[0] == 0:
            n_ctx_tiles += 1
            assert te[6] == row0_to_ctx[int(te[1])] and te[2] == cu_ctx[te[6] + 1] - cu_ctx[te[6]] and te[7] == 0
        else:
            assert te[6] == 0 and te[7] == 0
    # 85 queries of context 0, 165 of context 1, 64 query slots per tile
    assert [int(t[6]) for t in tiles if t[0] == 0] == [0, 0, 1, 1, 1] and n_ctx_tiles == 5
    # a context nobody names gets no tile; the numbers are the caller's, not a count of the contexts in use
    _, _, gap = plan_of(lib, [0, 5, 9], [2, 0], [0, 64, 192, 768], H=4, G=2)
    _, gt, _ = split_plan(gap)
    assert [(int(t[0]), int(t[1]), int(t[2]), int(t[6])) for t in gt] == [(0, 0, 64, 0), (0, 192, 576, 2), (1, 0, 5, 0), (1, 5, 4, 0)]


def test_plan_fields_of_the_existing_shapes_are_unchanged(lib):  # noqa: F811
    """the plan of test_captions_host.py's shapes, field by field against the layout rules of include/mjv.h: context tiles first
    (by context, 64 / G... 128 / G query slots per tile, first row = cu_context[c]), then own tiles sequence by sequence; parts
    consecutive; the only non-zero word in the two formerly free slots is te[6] of a context tile"""
    G, TR, H = 2, 128, 16
    QS, n_kv = TR // G, H // G
    own = [1, 200, 75, 33, 160, 7]
    index = [0, 1, 0, 0, 1, 0]
    q_lens = [1, 5, 75, 2, 160, 7]
    cu_seq, cu_q = np.concatenate([[0], np.cumsum(own)]), np.concatenate([[0], np.cumsum(q_lens)])
    cu_ctx = [0, 2112, 2112 + 576]
    n, ws, plan = plan_of(lib, cu_seq, index, cu_ctx, G=G, cu_q=cu_q)
    parts, tiles, _ = split_plan(plan)
    want_tiles, want_parts = [], []
    for c in range(2):
        q = sum(ql for ql, i in zip(q_lens, index) if i == c)
        nt, clen = -(-q // QS), cu_ctx[c + 1] - cu_ctx[c]
        kt = clen // 64
        want = max(1, min(-(-512 // (nt * n_kv)), 64, max(1, kt // 2)))
        chunk = -(-kt // want)
        split = -(-kt // chunk)
        for i in range(nt):
            want_tiles.append([0, cu_ctx[c], clen, len(want_parts), split, min(QS, q - i * QS) * G, c, 0])
            for s_ in range(split):
                want_parts.append([len(want_tiles) - 1, s_ * chunk * 64, min(clen, (s_ + 1) * chunk * 64), 0])
    for s_ in range(len(own)):
        ln, lq = own[s_], q_lens[s_]
        for q0 in range(0, lq, QS):
            nq = min(QS, lq - q0)
            want_tiles.append([1, int(cu_seq[s_]), ln, len(want_parts), 1, nq * G, 0, 0])
            want_parts.append([len(want_tiles) - 1, 0, min(ln, ln - lq + q0 + nq), 0])
    assert np.array_equal(tiles, np.asarray(want_tiles, dtype=np.int32))
    assert np.array_equal(parts, np.asarray(want_parts, dtype=np.int32))
    assert list(plan[:8]) == [0x43545837, len(want_parts), len(want_tiles), sum(q_lens), G, n_kv, 0, 0]
    assert ws == len(want_parts) * n_kv * TR * (128 + 2) * 4


def test_fresh_descriptor_names_no_lists():
    d = _lib.AttnCtxDesc()
    assert d.ctx_k_list is None and d.ctx_v_list is None and d.ctx_k is None and d.ctx_v is None
    names = [f[0] for f in _lib.AttnCtxDesc._fields_]
    assert names[-2:] == ["ctx_k_list", "ctx_v_list"] and names[-3] == "workspace_bytes", "the new fields go at the END of the struct"
    assert _lib.ABI_VERSION == 7


def test_head_dim_96_stays_refused(lib):  # noqa: F811
    """the Phi-3 tower is not part of this: the planner refuses head_dim 96 as before, and so do the model's entry points"""
    rc, msg, _ = plan_of(lib, [0, 5], [0], [0, 64], D=96)
    assert rc == -3 and "head_dim 96" in msg
    from mj_video_amd import configuration as C
    from mj_video_amd.modeling import InternVLChatRewardModeling
    cfg3 = C.InternVLChatRewardModelingConfig(**C.tiny_phi3_config_dict(56), **C.mjvideo_head_kwargs())
    m3 = InternVLChatRewardModeling.from_config(cfg3, dtype=BF)
    m3.model.img_context_token_id = synth.PHI3_TOKENS.img_context
    with pytest.raises(NotImplementedError, match="InternLM2 tower"):
        m3._caption_guard(torch.device("cuda:0"))


def host_model():
    from mj_video_amd.modeling import InternVLChatRewardModeling
    cfg, videos, prompts, index = cu.multi_case("tiny")
    model = InternVLChatRewardModeling.from_config(cfg, dtype=BF)
    model.config.pad_token_id = synth.PAD_ID
    model.model.img_context_token_id = synth.IMG_CONTEXT_ID
    first = [prompts[int(np.flatnonzero(index == v)[0])] for v in range(len(videos))]
    return model, videos, first


def test_encode_videos_host_checks_name_the_video():
    """``_analyse_videos`` is host code (as ``_analyse_captions`` is): what it derives, and every refusal with its video"""
    model, videos, prompts = host_model()
    info = model._analyse_videos(videos, prompts)
    per = model.model.num_image_token
    Ps = [x["P"] for x in info["videos"]]
    for v, (x, p) in enumerate(zip(info["videos"], prompts)):
        cols = np.flatnonzero(p[0].numpy() == synth.IMG_CONTEXT_ID)
        assert x["P"] == (int(cols[-1]) + 1) // 64 * 64 and x["n_img"] == videos[v].shape[0] * per == cols.size
        assert x["n_in"] == int((cols < x["P"]).sum()) and np.array_equal(x["ids"], p[0, :x["P"]].numpy())
    assert list(info["cu"]) == [0] + list(np.cumsum(Ps)) and info["total"] == sum(Ps) and info["max_len"] == max(Ps)
    assert info["N"] == max(p.shape[1] for p in prompts)
    assert np.array_equal(info["positions"], np.concatenate([np.arange(P) for P in Ps]))
    # every projected image row has exactly one destination: a context row that holds <IMG_CONTEXT>, or a tail row behind them
    rows = info["img_rows"]
    assert rows.size == sum(x["n_img"] for x in info["videos"]) and np.unique(rows).size == rows.size
    inside = rows[rows < info["total"]]
    assert (info["ids"][inside] == synth.IMG_CONTEXT_ID).all() and inside.size == int((info["ids"] == synth.IMG_CONTEXT_ID).sum())
    assert np.array_equal(np.sort(rows[rows >= info["total"]]), info["total"] + np.arange(int(info["cu_tail"][-1])))
    # [N] prompts and masks are taken as [1, N] ones are
    flat = model._analyse_videos(videos, [p[0] for p in prompts], [torch.ones(p.shape[1], dtype=torch.bool) for p in prompts])
    assert np.array_equal(flat["ids"], info["ids"]) and np.array_equal(flat["img_rows"], info["img_rows"])

    with pytest.raises(ValueError, match="empty list"):
        model._analyse_videos([], [])
    with pytest.raises(ValueError, match="3 videos, 2 prompts"):
        model._analyse_videos(videos, prompts[:2])
    with pytest.raises(ValueError, match="3 videos, 3 prompts, 1 attention masks"):
        model._analyse_videos(videos, prompts, [torch.ones_like(prompts[0])])
    with pytest.raises(ValueError, match=rf"video 1: {videos[1].shape[0] * per} <IMG_CONTEXT> tokens in input_ids but pixel_values holds {videos[1].shape[0] - 1} tiles"):
        model._analyse_videos([videos[0], videos[1][:-1], videos[2]], prompts)
    masks = [torch.ones_like(p) for p in prompts]
    masks[2][0, 17] = 0
    with pytest.raises(ValueError, match="video 2: masked column 17 inside the context"):
        model._analyse_videos(videos, prompts, masks)
    masks[2][0, 17] = 1
    masks[2][0, Ps[2]:] = 0                       # behind the context the mask is free
    model._analyse_videos(videos, prompts, masks)
    with pytest.raises(ValueError, match="video 0: attention_mask of"):
        model._analyse_videos(videos, prompts, [masks[0][:, :-1], masks[1], masks[2]])
    with pytest.raises(TypeError, match="video 1: pixel_values must be bfloat16"):
        model._analyse_videos([videos[0], videos[1].float(), videos[2]], prompts)
    with pytest.raises(ValueError, match="video 2: ONE prompt per video"):
        model._analyse_videos(videos, [prompts[0], prompts[1], prompts[2].repeat(2, 1)])
    with pytest.raises(ValueError, match="video 1: tiles of"):
        model._analyse_videos([videos[0], videos[1][:, :, :28], videos[2]], prompts)
    bad = prompts[0].clone()
    bad[0, 3] = -1
    with pytest.raises(IndexError, match="video 0: token id out of range"):
        model._analyse_videos(videos, [bad, prompts[1], prompts[2]])
    with pytest.raises(ValueError, match="SEQUENCES"):
        model._analyse_videos(videos[0], prompts[0])


def test_video_context_clone_and_sizes_on_the_host():
    """``clone()`` owns its rows; ``storage_nbytes`` counts what a view keeps alive, ``nbytes`` the view's own rows"""
    from mj_video_amd.modeling import VideoContext
    big_k, big_v, tails = torch.zeros(192, 8, dtype=BF), torch.zeros(192, 8, dtype=BF), torch.zeros(5, 4, dtype=BF)
    big_k[64:128] = 1
    view = VideoContext(np.arange(64), 64, [big_k[64:128]], [big_v[64:128]], tails[2:4], np.array([70, 71]), 9, ("s",), None, None,
                        torch.device("cpu"))
    assert view.nbytes == (2 * 64 * 8 + 2 * 4) * 2
    assert view.storage_nbytes == (2 * 192 * 8 + 5 * 4) * 2
    own = view.clone()
    assert own.nbytes == view.nbytes == own.storage_nbytes
    assert torch.equal(own.k[0], view.k[0]) and own.k[0].data_ptr() != view.k[0].data_ptr()
    assert own.settings == view.settings and own.P == 64 and own.n_img == 9 and np.array_equal(own.tail_cols, view.tail_cols)
    big_k[64:128] = 2
    assert float(own.k[0].float().max()) == 1.0, "a clone must not follow the buffer it was cut from"


def host_plan(ctx_lens=(64, 128), H=4, G=2):
    return ops.AttnCtxPlan([0, 3, 8], [1, 0], np.concatenate([[0], np.cumsum(ctx_lens)]), H, G, D, "cpu")


def test_attention_ctx_refuses_bad_context_tensors_before_any_launch(lib):  # noqa: F811
    """every context tensor is checked on the host before the C entry is reached (no GPU here: a call that got as far as the
    launch would fail on the HOST tensors with the TypeError of the last case, never with these messages)"""
    plan = host_plan()
    KV = 2
    q, o = torch.zeros(8, 4 * D, dtype=BF), torch.zeros(8, 4 * D, dtype=BF)
    k, v = torch.zeros(8, KV * D, dtype=BF), torch.zeros(8, KV * D, dtype=BF)
    ck = [torch.zeros(64, KV * D, dtype=BF), torch.zeros(128, KV * D, dtype=BF)]
    cv = [torch.zeros(64, KV * D, dtype=BF), torch.zeros(128, KV * D, dtype=BF)]

    def call(ck_, cv_, **kw):
        return ops.attention_ctx(q, k, v, o, ck_, cv_, plan, D ** -0.5, 2, None, **kw)

    odd = torch.zeros(128 * KV * D + 4, dtype=BF)[4:].view(128, KV * D)          # first row 8 bytes past a 16-byte boundary
    assert odd.data_ptr() % 16 == 8
    with pytest.raises(ValueError, match=r"context 1 \(keys\): its first row is not 16-byte aligned"):
        call([ck[0], odd], cv)
    with pytest.raises(ValueError, match=r"context 1 \(values\): 64 rows, the context has 128"):
        call(ck, [cv[0], cv[1][:64]])
    wide = torch.zeros(128, KV * D + 8, dtype=BF)[:, :KV * D]
    with pytest.raises(ValueError, match=r"context 1 \(keys\): leading dimension 264, context 0 has 256"):
        call([ck[0], wide], cv)
    with pytest.raises(ValueError, match=r"context 0 \(values\) lives on meta, the launch on cpu"):
        call(ck, [torch.empty(64, KV * D, dtype=BF, device="meta"), cv[1]])
    with pytest.raises(TypeError, match=r"context 0 \(keys\): expected bfloat16"):
        call([ck[0].float(), ck[1]], cv)
    with pytest.raises(ValueError, match=r"context 0 \(keys\): 128 columns do not hold 2 heads"):
        call([ck[0][:, :D], ck[1]], cv)
    with pytest.raises(ValueError, match="1 key / 2 value tensors for the plan's 2 contexts"):
        call(ck[:1], cv)
    with pytest.raises(ValueError, match="both be one packed tensor, or both a sequence"):
        call(ck, torch.cat(cv))
    with pytest.raises(ValueError, match="both be one packed tensor, or both a sequence"):
        call(torch.cat(ck), cv)
    with pytest.raises(ValueError, match=r"ctx_list must be a contiguous int64 tensor \[2, 2\]"):
        call(ck, cv, ctx_list=torch.zeros(2, 3, dtype=torch.int64))
    with pytest.raises(ValueError, match="ctx_list goes with per-context tensors"):
        call(torch.cat(ck), torch.cat(cv), ctx_list=torch.zeros(2, 2, dtype=torch.int64))
    rows = ops.ctx_pointer_rows(ck, cv)
    assert rows.dtype == np.int64 and rows.shape == (2, 2) and rows[1, 1] == cv[1].data_ptr()
    # good context tensors: the call goes on to the operands, which are host tensors here
    with pytest.raises(TypeError, match="expected a bf16 device tensor"):
        call(ck, cv)
    # the C entry itself: one list without the other is an argument error, decided before the plan or a pointer is looked at
    d = plan.desc()
    d.Q = d.K = d.V = d.O = 16
    d.ctx_k_list = 16
    assert lib.mjv_attention_ctx_bf16(C.byref(d), None) == -1 and b"both be given, or neither" in lib.mjv_last_error()
    d.ctx_k_list, d.ctx_v_list = None, 16
    assert lib.mjv_attention_ctx_bf16(C.byref(d), None) == -1 and b"both be given, or neither" in lib.mjv_last_error()
