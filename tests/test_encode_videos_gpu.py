"""Contexts where they lie (mjv_attn_ctx_desc.ctx_k_list / ctx_v_list) and ``model.encode_videos``: the launch over per-context
tensors against the packed launch of the same plan (equal bits) and the fp32 reference, ``encode_videos`` against
``encode_video`` video by video (equal bits at tiny dims, where no GEMM slices K: DESIGN §4.6), ``score_captions`` over views,
clones and both settings of ``caption_context_rows``, and the one shape with K-sliced GEMMs and cut contexts (2B dims) against
the stored fp32 oracle."""
import functools

import numpy as np
import pytest
import torch

import captions_util as cu_
import test_captions_gpu as tc
from test_e2e_gpu import ATOL_FLOOR
from util import FIELDS

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
D = 128
CTX_LENS = (64, 128, 576)
ARENA_ORDER = (2, 0, 1)       # the contexts by ascending address


@functools.lru_cache(maxsize=None)
def kernel_problem(H, n, suffix):
    """n sequences (own lengths 1 .. 70, both ends present from n = 2 on) over the three contexts, context_index 1, 0, 2, 1, ...;
    with ``suffix`` the last 1 .. 7 own rows are the queries.  One problem (and one fp32 reference per mode) per shape, shared
    by the tests below and left unchanged."""
    g = np.random.default_rng(100 + n)
    own = g.integers(1, 71, size=n).tolist()
    own[0] = 1
    if n > 1:
        own[-1] = 70
    index = [(2 * i + 1) % 3 for i in range(n)]
    q_lens = [min(L, 1 + (i * 3) % 7) for i, L in enumerate(own)] if suffix else None
    return tc.Problem(CTX_LENS, own, index, H, 2, q_lens, seed=30 + n)


@functools.lru_cache(maxsize=None)
def kernel_reference(H, n, suffix, mode):
    return kernel_problem(H, n, suffix).reference(mode)


def scattered(packed, cu_ctx, order, dev):
    """every context's rows as a tensor of its own at a known place: row blocks of one NaN-filled arena, two guard rows in front
    of / between / behind them, laid out in ``order`` (context numbers by ascending address).  A launch that reads a row outside
    a context's own tensor gets NaN."""
    lens = np.diff(cu_ctx)
    arena = torch.full((int(lens.sum()) + 2 * (len(lens) + 1), packed.shape[1]), float("nan"), dtype=BF, device=dev)
    out, r = [None] * len(lens), 2
    for c in order:
        out[c] = arena[r:r + int(lens[c])]
        out[c].copy_(packed[int(cu_ctx[c]):int(cu_ctx[c + 1])])
        r += int(lens[c]) + 2
    return out


def run_ctx(p, dev, mode, listed, contexts=None, seqs=None):
    """one launch of problem ``p``: ``listed`` - the contexts as separate tensors in ARENA order, else packed.  ``contexts``
    (context numbers, in the launch's order) / ``seqs``: a launch over a subset of p's sequences and contexts."""
    from mj_video_amd import ops
    contexts = list(range(len(p.ctx_lens))) if contexts is None else list(contexts)
    seqs = list(range(len(p.own_lens))) if seqs is None else list(seqs)
    own = [p.own_lens[s] for s in seqs]
    ql = [(p.q_lens if p.q_lens is not None else p.own_lens)[s] for s in seqs]
    cu, cu_q = (np.concatenate([[0], np.cumsum(a)]).astype(np.int32) for a in (own, ql))
    cu_ctx = np.concatenate([[0], np.cumsum([p.ctx_lens[c] for c in contexts])]).astype(np.int32)
    index = [contexts.index(p.index[s]) for s in seqs]
    rows = lambda t, c0, lst: torch.cat([t[c0[s]:c0[s + 1]] for s in lst]).to(dev)  # noqa: E731
    q, k, v = rows(p.q, p.cu_q, seqs), rows(p.k, p.cu, seqs), rows(p.v, p.cu, seqs)
    ck, cv = rows(p.ck, p.cu_ctx, contexts), rows(p.cv, p.cu_ctx, contexts)
    plan = ops.AttnCtxPlan(cu, index, cu_ctx, p.H, p.G, D, dev, cu_seqlens_q=cu_q if p.q_lens is not None else None)
    ws = torch.empty(plan.workspace_bytes, dtype=torch.uint8, device=dev)
    out = torch.full((int(cu_q[-1]) + 3, p.H * D), float("nan"), dtype=BF, device=dev)     # (+ 3 rows nobody may touch)
    if listed:
        order = [c for c in ARENA_ORDER if c < len(contexts)]
        order = order[::-1] if len(order) > 1 and order == sorted(order) else order
        lk, lv = scattered(ck, cu_ctx, order, dev), scattered(cv, cu_ctx, order, dev)
        ptr = [t.data_ptr() for t in lk]
        assert len(contexts) == 1 or sorted(ptr) != ptr, "the contexts must not lie in index order"
        ops.attention_ctx(q, k, v, out, lk, lv, plan, D ** -0.5, mode, ws)
    else:
        ops.attention_ctx(q, k, v, out, ck, cv, plan, D ** -0.5, mode, ws)
    torch.cuda.synchronize()
    return out.cpu(), cu_q


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("suffix", [False, True])
@pytest.mark.parametrize("n", [1, 3, 7])
@pytest.mark.parametrize("H", [4, 16])
def test_ctx_list_launch_equals_packed_launch_and_fp32(cuda, H, n, suffix, mode):
    """the same plan, the same arithmetic, other base pointers: equal bits; and the project's bound against fp32 (relative L2 <=
    4e-3, the bound of test_ctx_attention_vs_fp32)"""
    p = kernel_problem(H, n, suffix)
    packed, cu_q = run_ctx(p, cuda, mode, listed=False)
    listed, _ = run_ctx(p, cuda, mode, listed=True)
    nq = int(cu_q[-1])
    assert torch.equal(listed[:nq].view(torch.int16), packed[:nq].view(torch.int16)), "list launch and packed launch differ"
    assert torch.isnan(listed[nq:].float()).all(), "rows behind the queries were written"
    ref = kernel_reference(H, n, suffix, mode)
    got, want = listed[:nq].float(), ref.float()
    assert torch.isfinite(got).all()
    rel = ((got - want).norm() / want.norm()).item()
    print(f"H={H} n={n} suffix={suffix} mode={mode}: relative L2 to fp32 {rel:.3e}")
    assert rel <= 4e-3, rel


@pytest.mark.parametrize("suffix", [False, True])
@pytest.mark.parametrize("H", [4, 16])
def test_ctx_list_subset_in_permuted_order_keeps_every_sequences_bits(cuda, H, suffix):
    """the independence rule of DESIGN §4.8 for per-context tensors: a launch that names only contexts 2 and 0, in that order,
    with their sequences alone gives every one of those sequences the bits it has in the launch over all three"""
    for mode in (1, 2):
        p = kernel_problem(H, 7, suffix)
        full, cu_q = run_ctx(p, cuda, mode, listed=True)
        seqs = [s for s in range(7) if p.index[s] in (2, 0)]
        assert {p.index[s] for s in seqs} == {0, 2} and len(seqs) < 7
        sub, sub_cu = run_ctx(p, cuda, mode, listed=True, contexts=[2, 0], seqs=seqs)
        for j, s in enumerate(seqs):
            a, b = sub[sub_cu[j]:sub_cu[j + 1]], full[cu_q[s]:cu_q[s + 1]]
            assert torch.equal(a.view(torch.int16), b.view(torch.int16)), f"sequence {s} changed bits (mode {mode})"


# ------------------------------------------------------------------------------------------------------------------------
# model.encode_videos / score_captions over its views (tiny dims unless said)
TILES = (3, 16, 32)
CAPTION_LENGTHS = (5, 20, 41, 70)


@functools.lru_cache(maxsize=None)
def tiny_case():
    """three videos of 3 / 16 / 32 tiles @56^2 (contexts of 64 / 128 / 192 tokens) x four captions, rows caption-major"""
    from mj_video_amd import synth
    from mj_video_amd.chat_input import num_image_tokens_per_tile
    cfg = cu_.cfg_of("tiny")
    per = num_image_tokens_per_tile(cfg)
    videos = [synth.synth_pixel_values(55, v, t, 56) for v, t in enumerate(TILES)]
    prompts, index = [], []
    for j, L in enumerate(CAPTION_LENGTHS):
        for v, t in enumerate(TILES):
            prompts.append(synth.synth_input_ids(t * per, 700 + 4 * v + j, n_caption=L))
            index.append(v)
    ids, mask = synth.pad_batch(prompts)
    return cfg, videos, prompts, np.asarray(index, dtype=np.int64), ids, mask


def tiny_inputs(dev):
    cfg, videos, prompts, index, ids, mask = tiny_case()
    first = [prompts[int(np.flatnonzero(index == v)[0])] for v in range(len(videos))]
    return [v.to(dev) for v in videos], first, torch.from_numpy(index), ids.to(dev), mask.to(dev)


def same_outputs(a, b, what):
    for f in FIELDS:
        assert torch.equal(getattr(a, f), getattr(b, f)), (what, f)


def test_encode_videos_equals_encode_video_per_video(cuda):
    """every per-layer K and V and every img_tail of an ``encode_videos`` context, bit for bit what ``encode_video`` computes for
    that video alone (no GEMM slices K at these widths); V = 1 likewise; a context is a row range of the call's buffers"""
    model = tc.model_of("tiny", cuda)
    videos, first, index, ids, mask = tiny_inputs(cuda)
    singles = [model.encode_video(v, p) for v, p in zip(videos, first)]
    assert [c.P for c in singles] == [64, 128, 192]
    many = model.encode_videos(videos, first)
    alone = model.encode_videos(videos[1:2], first[1:2])
    torch.cuda.synchronize()
    assert len(many) == 3 and len(alone) == 1
    for v, (a, b) in enumerate(list(zip(many, singles)) + [(alone[0], singles[1])]):
        assert a.P == b.P and a.n_img == b.n_img and np.array_equal(a.ids, b.ids) and np.array_equal(a.tail_cols, b.tail_cols), v
        assert a.settings == b.settings and a.device == b.device and len(a.k) == len(b.k) == len(a.v) == len(b.v)
        for li in range(len(a.k)):
            assert a.k[li].shape == b.k[li].shape and torch.equal(a.k[li], b.k[li]), f"video {v}: keys of layer {li}"
            assert a.v[li].shape == b.v[li].shape and torch.equal(a.v[li], b.v[li]), f"video {v}: values of layer {li}"
        assert a.img_tail.shape == b.img_tail.shape and torch.equal(a.img_tail, b.img_tail), f"video {v}: img_tail"
        assert a.nbytes == b.nbytes == b.storage_nbytes
    # views of one buffer per layer: consecutive row ranges, and each keeps the whole call alive
    for li in range(len(many[0].k)):
        for t in ("k", "v"):
            base = getattr(many[0], t)[li]
            assert getattr(many[1], t)[li].data_ptr() == base.data_ptr() + 64 * base.stride(0) * 2
            assert getattr(many[2], t)[li].data_ptr() == base.data_ptr() + 192 * base.stride(0) * 2
    assert many[0].storage_nbytes == many[2].storage_nbytes >= sum(c.nbytes for c in many)
    assert alone[0].storage_nbytes == alone[0].nbytes


def test_score_captions_over_views_clones_and_both_row_modes(cuda):
    """``score_captions``: "in-place" == "packed" (bits); contexts of ``encode_videos`` == contexts of ``encode_video`` (bits); a view
    scores the same after its siblings are gone; a ``clone()`` scores the same and owns its rows"""
    model = tc.model_of("tiny", cuda)
    videos, first, index, ids, mask = tiny_inputs(cuda)
    singles = [model.encode_video(v, p) for v, p in zip(videos, first)]
    many = model.encode_videos(videos, first)
    try:
        assert model.caption_context_rows == "in-place"
        base = model.score_captions(singles, ids, mask, context_index=index)
        views = model.score_captions(many, ids, mask, context_index=index)
        model.caption_context_rows = "packed"
        packed = model.score_captions(singles, ids, mask, context_index=index)
        packed_views = model.score_captions(many, ids, mask, context_index=index)
        model.caption_context_rows = "in-place"
        same_outputs(base, packed, "in-place vs packed, contexts of encode_video")
        same_outputs(views, packed_views, "in-place vs packed, contexts of encode_videos")
        same_outputs(views, base, "contexts of encode_videos vs of encode_video")
        # mixed lists, in another order than the videos', are contexts like any other
        mixed = model.score_captions([many[2], singles[0], many[1]], ids, mask, context_index=torch.tensor([1, 2, 0] * 4))
        same_outputs(mixed, base, "mixed context list")
        model.caption_attention = "per-context"
        each = model.score_captions(many, ids, mask, context_index=index)
        model.caption_attention = "shared"
        assert torch.isfinite(each.score).all()
        # rows of video 1 alone, over the view, then over the view with its siblings deleted, then over a clone
        rows = torch.nonzero(index == 1).view(-1).to(cuda)
        one = model.score_captions(singles[1], ids[rows], mask[rows])
        keep = many[1]
        owned = keep.clone()
        assert owned.storage_nbytes == owned.nbytes == keep.nbytes < keep.storage_nbytes
        del many
        filler = [torch.full_like(singles[2].k[0], float("nan")) for _ in range(8)]   # (anything freed would be taken by these)
        same_outputs(model.score_captions(keep, ids[rows], mask[rows]), one, "a view after its siblings were deleted")
        del keep
        same_outputs(model.score_captions(owned, ids[rows], mask[rows]), one, "clone")
        del filler
        model.caption_context_rows = "gathered"
        with pytest.raises(ValueError, match="caption_context_rows 'gathered' not in"):
            model.score_captions(singles, ids, mask, context_index=index)
    finally:
        model.caption_context_rows, model.caption_attention = "in-place", "shared"


def test_encode_videos_runs_each_tower_once_whatever_v(cuda):
    """the profiler's view: one patchify launch and one attn_d64 launch per ViT layer per ``encode_videos`` call, one causal
    attention launch per decoder layer, for one video as for three"""
    from mj_video_amd import ops
    model = tc.model_of("tiny", cuda)
    cfg = cu_.cfg_of("tiny")
    videos, first, index, ids, mask = tiny_inputs(cuda)
    seen = []
    try:
        ops.prof_enable(True)
        for n in (1, 3):
            ops.prof_reset()
            model.encode_videos(videos[:n], first[:n])
            seen.append(ops.prof_results())
    finally:
        ops.prof_enable(False)
        ops.prof_reset()
    for tags in seen:
        assert tags["patchify"]["launches"] == 1 and tags["attn_d64"]["launches"] == cfg.vision_config.num_hidden_layers
        assert tags["attn_d128_causal"]["launches"] == cfg.llm_config.num_hidden_layers and "attn_ctx_d128" not in tags
    # (the GEMM tags name the tile a launch chose, which follows the row count: the number of launches does not)
    assert sum(v["launches"] for v in seen[0].values()) == sum(v["launches"] for v in seen[1].values())


def test_caption_matrix_in_blocks_of_videos(cuda):
    """harness.score_caption_matrix(videos_per_call=2) for 3 videos x 4 captions (blocks of 2 and 1 videos) under the bound of
    test_score_caption_matrix_equals_single_forwards: per block of the packed rows rms(matrix - fp32 oracle) <= 2 x rms(single
    forwards - fp32 oracle) + ATOL_FLOOR; and against the default path (videos_per_call = 1): equal bits at these dims"""
    from mj_video_amd import harness, synth
    from mj_video_amd.chat_input import prepare_chat_input, video_prefix
    from oracle import ref_cpu
    from test_host_logic import StubTokenizer
    model = tc.model_of("tiny", cuda)
    cfg = cu_.cfg_of("tiny")
    sd32 = {k: v.float() for k, v in synth.synth_state_dict(cfg, seed=0).items()}
    tok = StubTokenizer()
    videos = [synth.synth_pixel_values(31, v, t, 56) for v, t in enumerate((4, 3, 2))]
    captions = ["a cat walks over a red carpet", "two dogs", "the camera pans slowly over a harbour at dusk, boats", "x"]
    dv = [v.to(cuda) for v in videos]
    mat_t = harness.score_caption_matrix(model, cfg, tok, dv, captions, {}, max_rows=5, videos_per_call=2)
    default = harness.score_caption_matrix(model, cfg, tok, dv, captions, {}, max_rows=5)
    assert torch.equal(mat_t, default), "blocks of videos and one video per call differ"
    mat = mat_t.float().cpu().numpy()
    assert mat.shape == (3, 4, 34)
    with pytest.raises(ValueError, match="videos_per_call must be positive"):
        harness.score_caption_matrix(model, cfg, tok, dv, captions, {}, videos_per_call=0)
    singles, oracle = np.zeros_like(mat), np.zeros_like(mat)
    model.prefix_cache = False
    for v, pv in enumerate(videos):
        for j, c in enumerate(captions):
            ids, mask = prepare_chat_input(cfg, tok, pv, video_prefix(pv.shape[0]) + c, {}, device="cpu")
            model.forward(pv.to(cuda), ids.to(cuda), mask.to(cuda))
            singles[v, j] = model.last_packed34[0].float().cpu().numpy()
            ref = ref_cpu.reward_forward(sd32, cfg, pv.float(), ids, mask, synth.IMG_CONTEXT_ID, synth.PAD_ID)
            oracle[v, j] = np.concatenate([ref["score"].numpy().reshape(-1), ref["aspect_scores"].numpy().reshape(-1),
                                           ref["rewards"].float().numpy().reshape(-1)])
    nasp = model.num_aspects
    for name, sl in (("score", slice(0, 1)), ("aspect_scores", slice(1, 1 + nasp)), ("rewards", slice(1 + nasp, 34))):
        a, b = tc.rms(mat[..., sl] - oracle[..., sl]), tc.rms(singles[..., sl] - oracle[..., sl])
        print(f"matrix in blocks, {name}: rms(matrix - fp32 oracle) {a:.4e}, rms(single forwards - fp32 oracle) {b:.4e}")
        assert a <= 2 * b + ATOL_FLOOR, (name, a, b)


def test_encode_videos_2b_multi_vs_oracle(cuda):
    """MJ-VIDEO-2B dims @224^2, the ``multi`` case of tests/captions_util.py (contexts of 576 / 448 / 256 tokens): the one shape
    with K-sliced GEMMs (ff 8192) and cut contexts, so no bit claim - ``encode_videos`` + ``score_captions`` (contexts in place)
    against tests/golden/captions_2b_multi.npz with the bound of test_score_captions_vs_oracle_and_forward: per field
    rms(score_captions - fp32 oracle) <= 2 x rms(forward - fp32 oracle) + ATOL_FLOOR, the hidden rows' relative L2 to the oracle no
    more than 2 x forward's.  The profiler sees one patchify and 24 attn_d64 launches in the encode."""
    from mj_video_amd import ops
    model = tc.model_of("2b", cuda)
    cfg, videos, prompts, index, ids, mask, first = tc.case_tensors("2b", "multi", cuda)
    f32, _ = cu_.load_golden_captions("2b", "multi")
    try:
        ops.prof_enable(True)
        ops.prof_reset()
        ctxs = model.encode_videos(videos, [prompts[i] for i in first])
        enc = ops.prof_results()
    finally:
        ops.prof_enable(False)
        ops.prof_reset()
    assert [c.P for c in ctxs] == [576, 448, 256]
    assert enc["patchify"]["launches"] == 1 and enc["attn_d64"]["launches"] == 24
    assert model.caption_context_rows == "in-place" and model.caption_attention == "shared"
    out = model.score_captions(ctxs, ids, mask, context_index=torch.from_numpy(index))
    model.prefix_cache = False
    fw = model.forward(torch.cat([videos[int(c)] for c in index]), ids, mask)
    torch.cuda.synchronize()
    got = {f: getattr(out, f).float().cpu().numpy() for f in FIELDS}
    wit = {f: getattr(fw, f).float().cpu().numpy() for f in FIELDS}
    failures = []
    for f in tc.RMS_FIELDS:
        a, b = tc.rms(got[f] - f32[f]), tc.rms(wit[f] - f32[f])
        print(f"2b multi encode_videos {f}: rms(score_captions - fp32 oracle) {a:.4e}, rms(forward - fp32 oracle) {b:.4e}")
        if not a <= 2 * b + ATOL_FLOOR:
            failures.append((f, a, b))
    for f in tc.HIDDEN_FIELDS:
        a, b = tc.rel_l2(got[f], f32[f]), tc.rel_l2(wit[f], f32[f])
        print(f"2b multi encode_videos {f}: relative L2 to the fp32 oracle {a:.4e} (score_captions), {b:.4e} (forward)")
        if not a <= 2 * b:
            failures.append((f, a, b))
    assert not failures, failures
