"""model.extend_context / segmented VideoContexts end to end: a context that branches (one video, another
instruction) or grows (more frames) from a cached one without copying its rows, scored by model.score_captions next to plain
contexts and views - against the stored fp32 oracles of the caption cases (tests/golden/captions_*.npz) with the bound of
test_captions_gpu.py::test_score_captions_vs_oracle_and_forward, and the interface's refusals, sizes, lifetimes and streams."""
import gc

import numpy as np
import pytest
import torch

import captions_util as cu_
from test_captions_gpu import HIDDEN_FIELDS, RMS_FIELDS, case_tensors, model_of, rel_l2, rms
from test_e2e_gpu import ATOL_FLOOR
from util import FIELDS

pytestmark = pytest.mark.gpu
_WITNESS = {}


def witness_of(model, dims, case, dev):
    """``forward`` on the case's full prompts with prefix_cache = False, once per (dims, case): the second term of the bound"""
    if (dims, case) not in _WITNESS:
        cfg, videos, prompts, index, ids, mask, first = case_tensors(dims, case, dev)
        model.prefix_cache = False
        fw = model.forward(torch.cat([videos[int(c)] for c in index]), ids, mask)
        torch.cuda.synchronize()
        _WITNESS[dims, case] = {f: getattr(fw, f).float().cpu().numpy() for f in FIELDS}
        model.prefix_cache = True
    return _WITNESS[dims, case]


def check_bound(model, out, dims, case, dev, what, order=False):
    """per field rms(result - fp32 oracle) <= 2 x rms(forward - fp32 oracle) + ATOL_FLOOR, hidden rows: relative L2 to the
    oracle <= 2 x forward's; ``order``: no decisive pair of the fp32 oracle's scores is flipped"""
    f32, bf16 = cu_.load_golden_captions(dims, case)
    got = {f: getattr(out, f).float().cpu().numpy() for f in FIELDS}
    wit = witness_of(model, dims, case, dev)
    failures = []
    for f in RMS_FIELDS:
        a, b = rms(got[f] - f32[f]), rms(wit[f] - f32[f])
        print(f"{dims} {case} {what} {f}: rms(result - fp32 oracle) {a:.4e}, rms(forward - fp32 oracle) {b:.4e}")
        if not a <= 2 * b + ATOL_FLOOR:
            failures.append((f, a, b))
    for f in HIDDEN_FIELDS:
        a, b = rel_l2(got[f], f32[f]), rel_l2(wit[f], f32[f])
        print(f"{dims} {case} {what} {f}: relative L2 to the fp32 oracle {a:.4e} (result), {b:.4e} (forward)")
        if not a <= 2 * b:
            failures.append((f, a, b))
    assert not failures, (what, failures)
    if order:
        thr = 6 * rms(bf16["score"] - f32["score"])
        s32, s = f32["score"], got["score"]
        n = len(s32)
        pairs = [(i, j) for i in range(n) for j in range(i + 1, n) if abs(s32[i] - s32[j]) > thr]
        assert len(pairs) >= 24, f"only {len(pairs)} decisive pairs: the order check would be vacuous"
        flips = [(i, j) for i, j in pairs if (s32[i] > s32[j]) != (s[i] > s[j])]
        print(f"{dims} {what}: {len(pairs)} decisive pairs, flips {flips}")
        assert not flips, f"{what} orders {flips} against the fp32 oracle"


def kv_bytes(cfg, rows):
    lc = cfg.llm_config
    return 2 * rows * lc.num_key_value_heads * 128 * lc.num_hidden_layers * 2


def half_prompt(dims, tiles, seed, n_caption):
    """the synthetic prompt of a video's first ``tiles`` tiles"""
    from mj_video_amd import synth
    from mj_video_amd.chat_input import num_image_tokens_per_tile
    return synth.synth_input_ids(tiles * num_image_tokens_per_tile(cu_.cfg_of(dims)), seed, n_caption=n_caption)


@pytest.mark.parametrize("dims", ["tiny", "2b"])
def test_branch_one_video_under_another_instruction(cuda, dims):
    """encode_video (default rule) -> extend_context(text only) to the whole prefix the twelve prompts share -> score_captions:
    the bound of test_score_captions_vs_oracle_and_forward, no decisive pair flipped; the packed A/B partner within the same
    bound; no row of the parent copied"""
    from mj_video_amd import harness, synth
    model = model_of(dims, cuda)
    cfg, videos, prompts, index, ids, mask, first = case_tensors(dims, "one", cuda)
    parent = model.encode_video(videos[0], prompts[0])
    K = harness.shared_prefix_len(prompts, synth.PAD_ID)
    assert K > parent.P and K % 64
    child = model.extend_context(parent, prompts[0], context_len=K)
    assert child.P == K and len(child.segments) == 2 and len(parent.segments) == 1
    assert child.segments[0][0] is parent.k and child.segments[0][1] is parent.v and child.segments[0][2] == parent.P
    assert child.k[0].shape[0] == K - parent.P == child.segments[1][2] and child.n_img == parent.n_img
    assert np.array_equal(child.ids, prompts[0][0, :K].numpy()) and child.img_tail.shape[0] == 0 and child.tail_cols.size == 0
    # sizes: the branch adds its own rows; a clone would add the whole context
    assert child.nbytes == kv_bytes(cfg, K - parent.P) and parent.nbytes == kv_bytes(cfg, parent.P) + parent.img_tail.numel() * 2
    assert child.storage_nbytes == child.nbytes + kv_bytes(cfg, parent.P)
    assert parent.storage_nbytes == parent.nbytes, "a plain context keeps what it had"
    model.caption_context_rows = "in-place"
    out = model.score_captions(child, ids, mask)
    check_bound(model, out, dims, "one", cuda, "branch", order=True)
    model.caption_context_rows = "packed"
    try:
        packed = model.score_captions(child, ids, mask)
    finally:
        model.caption_context_rows = "in-place"
    check_bound(model, packed, dims, "one", cuda, "branch packed", order=True)
    # per-context reads one run of rows per context: a segmented one is refused by name, its clone is plain
    model.caption_attention = "per-context"
    try:
        with pytest.raises(ValueError, match=r"context 0 is segmented \(2 segments.*clone\(\)"):
            model.score_captions(child, ids, mask)
    finally:
        model.caption_attention = "shared"
    flat = child.clone()
    assert len(flat.segments) == 1 and flat.P == K and flat.nbytes == flat.storage_nbytes == kv_bytes(cfg, K)
    assert torch.equal(flat.k[-1], torch.cat([parent.k[-1], child.k[-1]])) and torch.equal(flat.v[0], torch.cat([parent.v[0], child.v[0]]))
    check_bound(model, model.score_captions(flat, ids, mask), dims, "one", cuda, "branch clone")


@pytest.mark.parametrize("dims,target", [("tiny", "shared"), ("tiny", 80), ("2b", None), ("2b", "shared")])
def test_grow_a_video_by_its_remaining_frames(cuda, dims, target):
    """parent: the first half of the tiles under a prompt for those tiles; extend_context with the remaining tiles and the full
    prompt (``target``: the default rule, an int inside the image run, or the whole shared prefix).  tiny: the parent's 64 tokens
    end before the image run, every image token comes from ``img_tail`` or the new tiles; 2b: 320 -> 576 tokens."""
    from mj_video_amd import harness, synth
    model = model_of(dims, cuda)
    cfg, videos, prompts, index, ids, mask, first = case_tensors(dims, "one", cuda)
    tiles = videos[0].shape[0]
    short = half_prompt(dims, tiles // 2, 500, cu_.ONE_LENGTHS[0])
    parent = model.encode_video(videos[0][:tiles // 2], short)
    assert np.array_equal(short[0, :parent.P].numpy(), prompts[0][0, :parent.P].numpy()), "the parent's ids are a prefix of the full prompt"
    K = harness.shared_prefix_len(prompts, synth.PAD_ID) if target == "shared" else target
    child = model.extend_context(parent, prompts[0], videos[0][tiles // 2:], context_len=K)
    cols = np.flatnonzero(prompts[0][0].numpy() == synth.IMG_CONTEXT_ID)
    want_P = K if K is not None else (int(cols[-1]) + 1) // 64 * 64
    n_in = int((cols < want_P).sum())
    assert child.P == want_P > parent.P and child.n_img == cols.size == 2 * parent.n_img
    assert child.img_tail.shape[0] == cols.size - n_in and np.array_equal(child.tail_cols, cols[n_in:])
    assert child.nbytes == kv_bytes(cfg, child.P - parent.P) + child.img_tail.numel() * 2
    assert child.storage_nbytes == child.nbytes + kv_bytes(cfg, parent.P)
    out = model.score_captions(child, ids, mask)
    check_bound(model, out, dims, "one", cuda, f"grow to {target}", order=True)
    flat = child.clone()
    assert len(flat.segments) == 1 and flat.img_tail.shape == child.img_tail.shape
    if flat.P % 64 == 0:
        model.caption_attention = "per-context"
    try:
        check_bound(model, model.score_captions(flat, ids, mask), dims, "one", cuda, f"grow to {target}, clone, {model.caption_attention}")
    finally:
        model.caption_attention = "shared"


def test_a_text_extension_runs_no_vision_kernel_and_only_the_new_rows(cuda):
    """library profiler, 2B dims: extend_context(pixel_values=None) launches no patchify / attn_d64, one segmented attention per
    layer, and GEMM flops of every Linear of every layer x the NEW rows (test 5 of test_captions_gpu.py counts the same terms)"""
    from mj_video_amd import harness, ops, synth
    dims = "2b"
    model = model_of(dims, cuda)
    cfg, videos, prompts, index, ids, mask, first = case_tensors(dims, "one", cuda)
    l = cfg.llm_config
    parent = model.encode_video(videos[0], prompts[0])
    K = harness.shared_prefix_len(prompts, synth.PAD_ID)
    try:
        ops.prof_enable(True)
        ops.prof_reset()
        child = model.extend_context(parent, prompts[0], context_len=K)
        ext = ops.prof_results()
    finally:
        ops.prof_enable(False)
        ops.prof_reset()
    assert "patchify" not in ext and "attn_d64" not in ext and "attn_d128_causal" not in ext, sorted(ext)
    assert ext["attn_ctx_d128"]["launches"] == l.num_hidden_layers
    rows = child.P - parent.P
    h, ff = l.hidden_size, l.intermediate_size
    hd = h // l.num_attention_heads
    per_tok = 2.0 * (h * (l.num_attention_heads + 2 * l.num_key_value_heads) * hd + l.num_attention_heads * hd * h + 3 * h * ff)
    gemm = sum(v["flops"] for k, v in ext.items() if k.startswith("gemm"))
    expect = l.num_hidden_layers * per_tok * rows
    print(f"new rows {rows}: GEMM flops {gemm:.4e}, per-row terms x rows {expect:.4e}, ratio {gemm / expect:.4f}")
    assert abs(gemm / expect - 1) < 0.01
    want = 4.0 * hd * l.num_hidden_layers * (rows * parent.P + rows * (rows + 1) / 2) * l.num_attention_heads
    assert abs(ext["attn_ctx_d128"]["flops"] / want - 1) < 1e-6


@pytest.mark.parametrize("dims", ["tiny", "2b"])
def test_chain_of_three_mixed_with_plain_contexts_and_views(cuda, dims):
    """multi case (videos of 8 / 6 / 3 tiles, 4 prompts each).  Video 0: first four tiles -> extend by the other four -> two
    children of THAT context, one to the whole shared prefix (a chain of three), one three tokens long.  Video 1: a view of
    encode_videos branched to its shared prefix, and a plain encode_video context.  Video 2: the view as it is.  One
    score_captions call, the rows of a video spread over its contexts, the parents dropped before it."""
    from mj_video_amd import harness, synth
    model = model_of(dims, cuda)
    cfg, videos, prompts, index, ids, mask, first = case_tensors(dims, "multi", cuda)
    rows_of = [[prompts[i] for i in np.flatnonzero(index == v)] for v in range(3)]
    shared = [harness.shared_prefix_len(r, synth.PAD_ID) for r in rows_of]
    end0 = int(np.flatnonzero(rows_of[0][0][0].numpy() == synth.IMG_CONTEXT_ID)[-1]) + 1
    p0 = model.encode_video(videos[0][:4], half_prompt(dims, 4, 600, cu_.MULTI_LENGTHS[0]))
    grown = model.extend_context(p0, rows_of[0][0], videos[0][4:], context_len=end0)
    c_long = model.extend_context(grown, rows_of[0][0], context_len=shared[0])
    c_short = model.extend_context(grown, rows_of[0][1], context_len=end0 + 3)
    views = model.encode_videos(videos[1:], [rows_of[1][0], rows_of[2][0]])
    c_branch = model.extend_context(views[0], rows_of[1][2], context_len=shared[1])
    c_plain = model.encode_video(videos[1], rows_of[1][0])
    c_view = views[1]
    assert [len(c.segments) for c in (c_long, c_short, c_branch, c_plain, c_view)] == [3, 3, 2, 1, 1]
    assert c_long.segments[1][0] is c_short.segments[1][0] is grown.k and c_long.segments[0][0] is p0.k
    assert c_long.storage_nbytes == c_long.nbytes + kv_bytes(cfg, grown.P)
    ctxs = [c_long, c_view, c_branch, c_short, c_plain]
    # rows of video 0 alternate between its two contexts, those of video 1 between the branch and the plain one
    seen = {0: 0, 1: 0, 2: 0}
    ci = []
    for v in index:
        ci.append({0: (0, 3), 1: (2, 4), 2: (1, 1)}[int(v)][seen[int(v)] % 2])
        seen[int(v)] += 1
    assert len(set(ci)) == 5
    del p0, grown, views
    gc.collect()
    torch.cuda.empty_cache()
    out = model.score_captions(ctxs, ids, mask, context_index=torch.tensor(ci))
    check_bound(model, out, dims, "multi", cuda, "chain of three, mixed")
    model.caption_context_rows = "packed"
    try:
        packed = model.score_captions(ctxs, ids, mask, context_index=torch.tensor(ci))
    finally:
        model.caption_context_rows = "in-place"
    check_bound(model, packed, dims, "multi", cuda, "chain of three, mixed, packed")
    again = model.score_captions(ctxs, ids, mask, context_index=torch.tensor(ci))
    for f in FIELDS:
        assert torch.equal(getattr(out, f), getattr(again, f)), f


def test_extend_context_refusals(cuda):
    from mj_video_amd import harness, synth
    dims = "tiny"
    model = model_of(dims, cuda)
    cfg, videos, prompts, index, ids, mask, first = case_tensors(dims, "one", cuda)
    parent = model.encode_video(videos[0], prompts[0])
    P, N = parent.P, prompts[0].shape[1]
    K = harness.shared_prefix_len(prompts, synth.PAD_ID)
    bad = prompts[0].clone()
    bad[0, 9] += 1

    def refused(match, *args, exc=ValueError, **kw):
        with pytest.raises(exc, match=match):
            model.extend_context(*args, **kw)

    refused(rf"first {P} token ids differ from those of the context to extend \(first at column 9\)", parent, bad, context_len=K)
    refused(rf"would hold {P} tokens, the context to extend holds {P} already", parent, prompts[0])          # default rule: 64 again
    refused(r"would hold 10 tokens", parent, prompts[0], context_len=10)
    for k in (0, N, -1, 64.0, True):
        refused("context_len must be None or an int", parent, prompts[0], context_len=k)
    refused(r"16 <IMG_CONTEXT> tokens in input_ids, but the context was built from 16 and pixel_values holds 1 new tiles",
            parent, prompts[0], videos[0][:1], context_len=K)
    refused("bfloat16", parent, prompts[0], videos[0][:1].float(), context_len=K, exc=TypeError)
    refused("first argument is the VideoContext", None, prompts[0], context_len=K)
    refused(rf"the prompt has {P} tokens", parent, prompts[0][:, :P], context_len=K)
    am = torch.ones(N, dtype=torch.long)
    am[P + 2] = 0
    refused(rf"masked column {P + 2} inside the context \({K} tokens\)", parent, prompts[0], attention_mask=am, context_len=K)
    model.extend_context(parent, prompts[0], attention_mask=am, context_len=P + 2)
    model.attention_scores = "eager" if model.attention_scores == "flash" else "flash"
    try:
        refused("built under other settings", parent, prompts[0], context_len=K)
    finally:
        model.attention_scores = "eager" if model.attention_scores == "flash" else "flash"
    child = model.extend_context(parent, prompts[0], context_len=K)
    sd = model.state_dict()
    model.load_state_dict(sd, strict=True)                        # new weights (same values: the versions moved)
    refused("built under other settings", parent, prompts[0], context_len=K)
    with pytest.raises(ValueError, match="context 0 was built under other settings"):
        model.score_captions(child, *(t.to(cuda) for t in synth.pad_batch(prompts)))


def test_a_child_built_on_another_stream_waits_for_its_parent(cuda):
    """the pattern of test_context_on_another_stream_waits_for_its_event: the parent is encoded on the main stream behind a
    long-running kernel; with no synchronise in between a side stream extends it and scores.  Only the parent's ready-event
    orders the two; the child's own event orders the scoring pass on yet another stream.  Other pixels every round."""
    from mj_video_amd import harness, synth
    model = model_of("tiny", cuda)
    cfg, videos, prompts, index, ids, mask, first = case_tensors("tiny", "one", cuda)
    K = harness.shared_prefix_len(prompts, synth.PAD_ID)
    px = [synth.synth_pixel_values(300 + r, 0, 4, 56).to(cuda) for r in range(2)]
    expect = []
    for p in px:
        child = model.extend_context(model.encode_video(p[:2], half_prompt("tiny", 2, 500, 1)), prompts[0], p[2:], context_len=K)
        expect.append(model.score_captions(child, ids, mask))
        torch.cuda.synchronize()
    assert not torch.equal(expect[0].score, expect[1].score)
    for r, p in enumerate(px):
        torch.cuda.synchronize()
        torch.cuda._sleep(400_000_000)
        parent = model.encode_video(p[:2], half_prompt("tiny", 2, 500, 1))
        assert not parent.ready.query(), "the parent's rows must still be pending when the side stream starts"
        s1, s2 = torch.cuda.Stream(device=cuda), torch.cuda.Stream(device=cuda)
        with torch.cuda.stream(s1):
            child = model.extend_context(parent, prompts[0], p[2:], context_len=K)
        assert child.stream == s1.cuda_stream != parent.stream
        del parent
        with torch.cuda.stream(s2):
            got = model.score_captions(child, ids, mask)
        s2.synchronize()
        for f in FIELDS:
            assert torch.equal(getattr(got, f), getattr(expect[r], f)), (r, f)
        torch.cuda.synchronize()


def test_score_growing_video_equals_single_forwards(cuda):
    """harness.score_growing_video at lengths 2 / 4 / 8 against single ``forward``s of the first 2 / 4 / 8 frames, with the bound
    of test_score_caption_matrix_equals_single_forwards: per block of the packed rows rms(growing - fp32 oracle) <=
    2 x rms(single forwards - fp32 oracle) + ATOL_FLOOR (the oracle at tiny dims runs here)"""
    from mj_video_amd import harness, ops, synth
    from mj_video_amd.chat_input import prepare_chat_input, video_prefix
    from oracle import ref_cpu
    from test_host_logic import StubTokenizer
    model = model_of("tiny", cuda)
    cfg = cu_.cfg_of("tiny")
    sd32 = {k: v.float() for k, v in synth.synth_state_dict(cfg, seed=0).items()}
    tok = StubTokenizer()
    video = synth.synth_pixel_values(41, 0, 8, 56)
    captions = ["a cat walks over a red carpet", "two dogs", "the camera pans slowly over a harbour at dusk, boats"]
    lengths = (2, 4, 8)
    try:
        ops.prof_enable(True)
        ops.prof_reset()
        got = harness.score_growing_video(model, cfg, tok, video.to(cuda), captions, {}, lengths=lengths)
        prof = ops.prof_results()
    finally:
        ops.prof_enable(False)
        ops.prof_reset()
    assert prof["patchify"]["launches"] == len(lengths), "the vision tower runs once per step, on the new frames alone"
    got = got.float().cpu().numpy()
    assert got.shape == (3, 3, 34)
    singles, oracle = np.zeros_like(got), np.zeros_like(got)
    model.prefix_cache = False
    for i, n in enumerate(lengths):
        pv = video[:n]
        for j, c in enumerate(captions):
            ids, mask = prepare_chat_input(cfg, tok, pv, video_prefix(n) + c, {}, device="cpu")
            model.forward(pv.to(cuda), ids.to(cuda), mask.to(cuda))
            singles[i, j] = model.last_packed34[0].float().cpu().numpy()
            ref = ref_cpu.reward_forward(sd32, cfg, pv.float(), ids, mask, synth.IMG_CONTEXT_ID, synth.PAD_ID)
            oracle[i, j] = np.concatenate([ref["score"].numpy().reshape(-1), ref["aspect_scores"].numpy().reshape(-1),
                                           ref["rewards"].float().numpy().reshape(-1)])
    nasp = model.num_aspects
    for name, sl in (("score", slice(0, 1)), ("aspect_scores", slice(1, 1 + nasp)), ("rewards", slice(1 + nasp, 34))):
        a, b = rms(got[..., sl] - oracle[..., sl]), rms(singles[..., sl] - oracle[..., sl])
        print(f"growing {name}: rms(growing - fp32 oracle) {a:.4e}, rms(single forwards - fp32 oracle) {b:.4e}")
        assert a <= 2 * b + ATOL_FLOOR, (name, a, b)
    with pytest.raises(ValueError, match="must ascend strictly"):
        harness.score_growing_video(model, cfg, tok, video.to(cuda), captions, {}, lengths=(4, 2))
    with pytest.raises(ValueError, match="must ascend strictly"):
        harness.score_growing_video(model, cfg, tok, video.to(cuda), captions, {}, lengths=(4, 9))
