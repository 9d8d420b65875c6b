"""Video contexts of any length on the MI355X: mjv_attention_ctx_bf16 with ``ctx_any_length`` against the fp32 reference on the
concatenated [context | own] rows (the ``Problem`` pattern of tests/test_captions_gpu.py, restated with per-sequence tensors so
that launches can be combined), that no row behind a context's length is used, flag on == flag off on whole-tile contexts; and
``model.encode_video(s)(..., context_len=...)`` / ``score_captions`` / ``harness.score_caption_matrix(context="shared")`` against the
stored fp32 oracle (tests/golden/captions_*.npz: scores of the full prompts, whatever the context holds)."""
import functools

import numpy as np
import pytest
import torch

import captions_util as cu_
from test_captions_gpu import HIDDEN_FIELDS, RMS_FIELDS, attn_reference_rows, case_tensors, model_of, rel_l2, rms
from test_e2e_gpu import ATOL_FLOOR
from test_kernels_gpu import rnd
from util import FIELDS

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
D = 128


class Problem:
    """one launch on the host (bf16): per context its keys / values, per sequence its context number, own keys / values and
    queries (the LAST rows of the sequence)"""

    def __init__(self, H, G, ctx, seqs):
        self.H, self.G, self.ctx, self.seqs = H, G, list(ctx), list(seqs)     # ctx: (ck, cv); seqs: (context, q, k, v)

    @classmethod
    def random(cls, ctx_lens, own_lens, index, H, G, q_lens=None, seed=0):
        KV = H // G
        ctx = [(rnd(L, KV * D, seed=seed + 100 + 2 * c), rnd(L, KV * D, seed=seed + 101 + 2 * c)) for c, L in enumerate(ctx_lens)]
        seqs = []
        for s, L in enumerate(own_lens):
            lq = L if q_lens is None else q_lens[s]
            seqs.append((index[s], rnd(lq, H * D, seed=seed + 1000 + 3 * s), rnd(L, KV * D, seed=seed + 1001 + 3 * s),
                         rnd(L, KV * D, seed=seed + 1002 + 3 * s)))
        return cls(H, G, ctx, seqs)

    @property
    def cu_q(self):
        return np.concatenate([[0], np.cumsum([s[1].shape[0] for s in self.seqs])]).astype(np.int32)

    @property
    def ctx_lens(self):
        return [c[0].shape[0] for c in self.ctx]

    def reference(self, mode):
        """fp32 attention of every sequence's queries on [its context | its own rows], rounded to bf16"""
        return torch.cat([attn_reference_rows(q, torch.cat([self.ctx[c][0], k]), torch.cat([self.ctx[c][1], v]), self.H, self.G,
                                              D ** -0.5, mode) for c, q, k, v in self.seqs])

    def run(self, dev, mode, any_length=True, listed=False, fill=float("nan"), unnamed_fill=None):
        """``listed``: every context a slice of its own of an arena filled with ``fill`` (two guard rows around each), else the
        packed buffers; ``unnamed_fill``: packed rows of contexts that no sequence names are overwritten with it"""
        from mj_video_amd import ops
        own = [s[2].shape[0] for s in self.seqs]
        cu = np.concatenate([[0], np.cumsum(own)]).astype(np.int32)
        cu_q, lens = self.cu_q, self.ctx_lens
        cu_ctx = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        suffix = any(s[1].shape[0] != s[2].shape[0] for s in self.seqs)
        plan = ops.AttnCtxPlan(cu, [s[0] for s in self.seqs], cu_ctx, self.H, self.G, D, dev, cu_seqlens_q=cu_q if suffix else None,
                               any_length=any_length)
        ws = torch.empty(plan.workspace_bytes, dtype=torch.uint8, device=dev)
        nq = int(cu_q[-1])
        out = torch.full((nq + 3, self.H * D), float("nan"), dtype=BF, device=dev)     # (+ 3 rows nobody may touch)
        q, k, v = (torch.cat([s[i] for s in self.seqs]).to(dev) for i in (1, 2, 3))
        if listed:
            KV = self.H // self.G
            arena = torch.full((2, sum(lens) + 2 * (len(lens) + 1), KV * D), fill, dtype=BF, device=dev)
            lk, lv, r = [], [], 2
            for ck, cv in self.ctx:
                lk.append(arena[0, r:r + ck.shape[0]].copy_(ck))
                lv.append(arena[1, r:r + cv.shape[0]].copy_(cv))
                r += ck.shape[0] + 2
            ops.attention_ctx(q, k, v, out, lk, lv, plan, D ** -0.5, mode, ws)
        else:
            ck, cv = (torch.cat([c[i] for c in self.ctx]).to(dev) for i in (0, 1))
            if unnamed_fill is not None:
                named = {s[0] for s in self.seqs}
                for c in range(len(lens)):
                    if c not in named:
                        ck[cu_ctx[c]:cu_ctx[c + 1]] = unnamed_fill
                        cv[cu_ctx[c]:cu_ctx[c + 1]] = unnamed_fill
            ops.attention_ctx(q, k, v, out, ck, cv, plan, D ** -0.5, mode, ws)
        torch.cuda.synchronize()
        out = out.cpu()
        assert torch.isnan(out[nq:].float()).all(), "rows behind the queries were written"
        return out[:nq]


def own_lengths(n, seed):
    """own lengths from 1 to 200, both ends present"""
    g = np.random.default_rng(seed)
    lens = g.integers(1, 201, size=n).tolist()
    lens[0] = 1
    if n > 1:
        lens[-1] = 200
    return lens


@functools.lru_cache(maxsize=None)
def make_problem(ctx_lens, n, H, G, suffix, seed=10):
    own = own_lengths(n, seed)
    index = [i % len(ctx_lens) for i in range(n)]
    q_lens = [min(L, 1 + (i * 3) % 7) for i, L in enumerate(own)] if suffix else None
    return Problem.random(ctx_lens, own, index, H, G, q_lens, seed=seed)


@functools.lru_cache(maxsize=None)
def reference_of(ctx_lens, n, H, G, suffix, mode):
    """one fp32 reference per shape and mode, shared by the tests below and left unchanged"""
    return make_problem(ctx_lens, n, H, G, suffix).reference(mode)


def bits(t):
    return t.contiguous().view(torch.int16)


# (context lengths, sequences, H, G, suffix queries)
SHAPES = [
    ((33,), 1, 4, 2, False),
    ((1,), 3, 4, 2, False),
    ((63, 65), 5, 16, 2, True),
    ((100,), 7, 16, 2, False),
    ((613,), 5, 16, 2, True),
    ((2149,), 2, 16, 2, False),
    ((2149, 576, 293), 7, 4, 2, True),
]


@pytest.mark.parametrize("listed", [False, True], ids=["packed", "lists"])
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("ctx_lens,n,H,G,suffix", SHAPES)
def test_ragged_contexts_vs_fp32(cuda, ctx_lens, n, H, G, suffix, mode, listed):
    """the error model of test_ctx_attention_vs_fp32 (P rounded before against after normalisation; fp32 partials merged by exact
    powers of two): masking the keys behind a context's end adds no rounding point, so the project's bound, relative L2 < 4e-3"""
    p = make_problem(ctx_lens, n, H, G, suffix)
    got, want = p.run(cuda, mode, listed=listed).float(), reference_of(ctx_lens, n, H, G, suffix, mode).float()
    assert torch.isfinite(got).all(), "NaN / inf left in query rows"
    rel = ((got - want).norm() / want.norm()).item()
    print(f"ctx{ctx_lens} n={n} H={H} suffix={suffix} mode={mode} listed={listed}: relative L2 {rel:.3e}")
    assert rel < 4e-3, rel


@pytest.mark.parametrize("mode", [1, 2])
def test_rows_behind_a_length_are_not_used(cuda, mode):
    """packed [100, 64] with no sequence naming context 1: whatever its rows hold (NaN, zeros) the output is finite and the same
    bits - rows 100 .. 127 of the packed buffer, which context 0's last key tile would cover, are never used.  Lists: the
    contexts are slices of one allocation filled with NaN, or with zeros."""
    own = own_lengths(5, 2)
    p = Problem.random((100, 64), own, [0] * 5, 16, 2, seed=50)
    a, b = p.run(cuda, mode, unnamed_fill=float("nan")), p.run(cuda, mode, unnamed_fill=0.0)
    assert torch.isfinite(a.float()).all() and torch.equal(bits(a), bits(b))
    for ctx_lens, index in (((100, 64), [0, 1, 0, 1, 0]), ((1, 613, 33), [2, 0, 1, 1, 2])):
        p = Problem.random(ctx_lens, own, index, 16, 2, seed=51)
        a, b = p.run(cuda, mode, listed=True, fill=float("nan")), p.run(cuda, mode, listed=True, fill=0.0)
        assert torch.isfinite(a.float()).all() and torch.equal(bits(a), bits(b))
        assert torch.equal(bits(a), bits(p.run(cuda, mode))), "lists and packed buffers differ"


@pytest.mark.parametrize("ctx_lens,n", [((64,), 5), ((2112, 576), 7)])
def test_flag_on_equals_flag_off_on_whole_tiles(cuda, ctx_lens, n):
    for suffix in (False, True):
        p = make_problem(ctx_lens, n, 16, 2, suffix, seed=12)
        for mode in (1, 2):
            for listed in (False, True):
                on, off = p.run(cuda, mode, any_length=True, listed=listed), p.run(cuda, mode, any_length=False, listed=listed)
                assert torch.equal(bits(on), bits(off)), (suffix, mode, listed)


@pytest.mark.parametrize("mode", [1, 2])
def test_ragged_context_equals_whole_tiles_plus_own_rows(cuda, mode):
    """a check of this file's own layout: [613] as the launch before this flag would take it - a context of 576 keys, the other 37
    prepended to every sequence's own rows, cu_seqlens_q selecting the original queries.  Two fp32 associations of one
    function, both held to fp32 at 4e-3 elsewhere: relative L2 between them < 4e-3."""
    p = make_problem((613,), 5, 16, 2, True)
    ck, cv = p.ctx[0]
    old = Problem(p.H, p.G, [(ck[:576], cv[:576])], [(0, q, torch.cat([ck[576:], k]), torch.cat([cv[576:], v])) for _, q, k, v in p.seqs])
    a, b = p.run(cuda, mode).float(), old.run(cuda, mode, any_length=False).float()
    rel = ((a - b).norm() / b.norm()).item()
    print(f"[613] against [576] + 37 own rows, mode {mode}: relative L2 {rel:.3e}")
    assert rel < 4e-3, rel


def test_ragged_equal_bits_and_independence(cuda):
    """two launches give equal bits; the sequences of a ragged context keep their bits when another context's join the launch"""
    alone = Problem.random((2149,), own_lengths(4, 3), [0] * 4, 16, 2, seed=20)
    other = Problem.random((613,), own_lengths(3, 4), [0] * 3, 16, 2, seed=40)
    for mode in (1, 2):
        a1, a2 = alone.run(cuda, mode), alone.run(cuda, mode)
        assert torch.equal(bits(a1), bits(a2))
        order = [(0, 0), (1, 0), (0, 1), (1, 1), (1, 2), (0, 2), (0, 3)]
        seqs = [((src,) + (alone, other)[src].seqs[j][1:]) for src, j in order]
        both = Problem(16, 2, [alone.ctx[0], other.ctx[0]], seqs)
        m, o = both.run(cuda, mode), other.run(cuda, mode)
        for pos, (src, j) in enumerate(order):
            want, cu = ((a1, alone.cu_q), (o, other.cu_q))[src]
            got = m[both.cu_q[pos]:both.cu_q[pos + 1]]
            assert torch.equal(bits(got), bits(want[cu[j]:cu[j + 1]])), f"sequence {j} of context {src} changed bits (mode {mode})"


# ------------------------------------------------------------------------------------------------------------------------
# model.encode_video / encode_videos with ``context_len``, score_captions, the harness
SHARED = {("tiny", "one"): [117], ("tiny", "multi"): [133, 125, 113], ("2b", "one"): [613], ("2b", "multi"): [613, 485, 293]}


def video_ends(prompts, first):
    from mj_video_amd import synth
    return [int(np.flatnonzero(prompts[i][0].numpy() == synth.IMG_CONTEXT_ID)[-1]) + 1 for i in first]


def same_context(a, b, what):
    assert a.P == b.P and a.n_img == b.n_img and np.array_equal(a.ids, b.ids) and np.array_equal(a.tail_cols, b.tail_cols), what
    assert a.settings == b.settings and len(a.k) == len(b.k) == len(a.v) == len(b.v)
    for li in range(len(a.k)):
        assert torch.equal(a.k[li], b.k[li]) and torch.equal(a.v[li], b.v[li]), f"{what}: layer {li}"
    assert a.img_tail.shape == b.img_tail.shape and torch.equal(a.img_tail, b.img_tail), f"{what}: img_tail"


def same_outputs(a, b, what):
    for f in FIELDS:
        assert torch.equal(getattr(a, f), getattr(b, f)), (what, f)


def test_context_len_64_is_the_default_context_at_tiny_dims(cuda):
    """tiny dims, one video: the video ends at column 87, so today's rule gives P = 64 - and ``context_len=64`` the same bits"""
    model = model_of("tiny", cuda)
    cfg, videos, prompts, index, ids, mask, first = case_tensors("tiny", "one", cuda)
    a, b = model.encode_video(videos[0], prompts[0]), model.encode_video(videos[0], prompts[0], context_len=64)
    assert a.P == 64 and video_ends(prompts, first) == [87]
    same_context(a, b, "context_len=64")
    same_outputs(model.score_captions(a, ids, mask), model.score_captions(b, ids, mask), "context_len=64")


def test_encode_videos_with_lengths_views_clones_and_row_modes(cuda):
    """tiny dims (no GEMM slices K), three videos with their shared-prefix lengths 133 / 125 / 113: ``encode_videos`` == ``encode_video``
    per video, "in-place" == "packed", views == clones - all bit for bit; the views start at rows 133 and 258 of the call's buffers"""
    model = model_of("tiny", cuda)
    cfg, videos, prompts, index, ids, mask, first = case_tensors("tiny", "multi", cuda)
    lens = SHARED["tiny", "multi"]
    idx = torch.from_numpy(index)
    singles = [model.encode_video(v, prompts[first[i]], context_len=lens[i]) for i, v in enumerate(videos)]
    many = model.encode_videos(videos, [prompts[i] for i in first], context_len=lens)
    assert [c.P for c in many] == lens
    for v in range(3):
        same_context(many[v], singles[v], f"video {v}")
    base0 = many[0].k[0]
    assert many[1].k[0].data_ptr() == base0.data_ptr() + 133 * base0.stride(0) * 2
    assert many[2].v[-1].data_ptr() == many[0].v[-1].data_ptr() + 258 * many[0].v[-1].stride(0) * 2
    one_len = model.encode_videos(videos, [prompts[i] for i in first], context_len=100)
    assert [c.P for c in one_len] == [100] * 3
    same_context(one_len[1], model.encode_video(videos[1], prompts[first[1]], context_len=100), "one int for every video")
    try:
        assert model.caption_context_rows == "in-place"
        base = model.score_captions(singles, ids, mask, context_index=idx)
        views = model.score_captions(many, ids, mask, context_index=idx)
        clones = model.score_captions([c.clone() for c in many], ids, mask, context_index=idx)
        model.caption_context_rows = "packed"
        packed = model.score_captions(many, ids, mask, context_index=idx)
    finally:
        model.caption_context_rows = "in-place"
    same_outputs(views, base, "contexts of encode_videos vs of encode_video")
    same_outputs(clones, views, "clones vs views")
    same_outputs(packed, views, "packed vs in-place")


@functools.lru_cache(maxsize=None)
def forward_witness(dims, case):
    """``forward`` on the full prompts with prefix_cache = False (the second witness of test_score_captions_vs_oracle_and_forward),
    once per case"""
    dev = torch.device("cuda:0")
    model = model_of(dims, dev)
    cfg, videos, prompts, index, ids, mask, first = case_tensors(dims, case, dev)
    model.prefix_cache = False
    fw = model.forward(torch.cat([videos[int(c)] for c in index]), ids, mask)
    torch.cuda.synchronize()
    model.prefix_cache = True
    return {f: getattr(fw, f).float().cpu().numpy() for f in FIELDS}


def check_oracle_bound(got, wit, f32, what):
    failures = []
    for f in RMS_FIELDS:
        a, b = rms(got[f] - f32[f]), rms(wit[f] - f32[f])
        print(f"{what} {f}: rms(score_captions - fp32 oracle) {a:.4e}, rms(forward - fp32 oracle) {b:.4e}")
        if not a <= 2 * b + ATOL_FLOOR:
            failures.append((f, a, b))
    for f in HIDDEN_FIELDS:
        a, b = rel_l2(got[f], f32[f]), rel_l2(wit[f], f32[f])
        print(f"{what} {f}: relative L2 to the fp32 oracle {a:.4e} (score_captions), {b:.4e} (forward)")
        if not a <= 2 * b:
            failures.append((f, a, b))
    assert not failures, failures


@pytest.mark.parametrize("where", ["shared", "video_end"])
@pytest.mark.parametrize("case", ["one", "multi"])
@pytest.mark.parametrize("dims", ["tiny", "2b"])
def test_score_captions_over_ragged_contexts_vs_oracle(cuda, dims, case, where):
    """the bound of test_score_captions_vs_oracle_and_forward, unchanged, for contexts that hold the whole shared prefix and for
    contexts that end exactly with the video (87 / 583 in the one-video cases; ``img_tail`` empty): per field rms(score_captions -
    fp32 oracle) <= 2 x rms(forward - fp32 oracle) + ATOL_FLOOR, the hidden rows' relative L2 no more than 2 x forward's, and no
    decisive pair of the one-video case ordered against the oracle.  One video: ``encode_video``; three: ``encode_videos``."""
    model = model_of(dims, cuda)
    cfg, videos, prompts, index, ids, mask, first = case_tensors(dims, case, cuda)
    f32, bf16 = cu_.load_golden_captions(dims, case)
    ends = video_ends(prompts, first)
    if case == "one":
        assert ends == [{"tiny": 87, "2b": 583}[dims]]
    lens = SHARED[dims, case] if where == "shared" else ends
    assert any(L % 64 for L in lens)
    if case == "one":
        ctxs = [model.encode_video(videos[0], prompts[0], context_len=lens[0])]
    else:
        ctxs = model.encode_videos(videos, [prompts[i] for i in first], context_len=lens)
    assert [c.P for c in ctxs] == lens
    if where == "video_end":
        assert all(c.img_tail.shape[0] == 0 and c.tail_cols.size == 0 for c in ctxs)
    out = model.score_captions(ctxs, ids, mask, context_index=torch.from_numpy(index))
    torch.cuda.synchronize()
    got = {f: getattr(out, f).float().cpu().numpy() for f in FIELDS}
    check_oracle_bound(got, forward_witness(dims, case), f32, f"{dims} {case} {where}")
    if case == "one":
        thr = 6 * rms(bf16["score"] - f32["score"])
        s32, s = f32["score"], got["score"]
        n = len(s32)
        pairs = [(i, j) for i in range(n) for j in range(i + 1, n) if abs(s32[i] - s32[j]) > thr]
        assert len(pairs) >= 24, f"only {len(pairs)} decisive pairs: the order check would be vacuous"
        flips = [(i, j) for i, j in pairs if (s32[i] > s32[j]) != (s[i] > s[j])]
        assert not flips, f"score_captions orders {flips} against the fp32 oracle"


def test_shared_context_leaves_the_common_rows_out(cuda):
    """2B dims, one video under twelve captions: with the context at the prompts' common prefix (613 tokens) the call's caption
    rows are 682 against 1 126 under today's rule (P = 576), and the profiler's GEMM flops are the per-row terms of
    test_score_captions_leaves_the_shared_work_out x 682, within its 1 %"""
    from mj_video_amd import ops
    model = model_of("2b", cuda)
    cfg, videos, prompts, index, ids, mask, first = case_tensors("2b", "one", cuda)
    l = cfg.llm_config
    ctx = model.encode_video(videos[0], prompts[0], context_len=613)
    try:
        ops.prof_enable(True)
        ops.prof_reset()
        model.score_captions(ctx, ids, mask)
        cap = ops.prof_results()
    finally:
        ops.prof_enable(False)
        ops.prof_reset()
    rows = sum(p.shape[1] - ctx.P for p in prompts)
    assert rows == 682 and sum(p.shape[1] - 576 for p in prompts) == 1126
    assert "attn_d64" not in cap and "patchify" not in cap and "attn_d128_causal" not in cap, sorted(cap)
    assert cap["attn_ctx_d128"]["launches"] == l.num_hidden_layers
    h, ff = l.hidden_size, l.intermediate_size
    hd = h // l.num_attention_heads
    qkv_out, kv_out = (l.num_attention_heads + 2 * l.num_key_value_heads) * hd, 2 * l.num_key_value_heads * hd
    per_tok = 2.0 * (h * qkv_out + l.num_attention_heads * hd * h + 3 * h * ff)
    expect = ((l.num_hidden_layers - 1) * per_tok + 2.0 * h * kv_out) * rows
    gemm = sum(v["flops"] for k, v in cap.items() if k.startswith("gemm"))
    print(f"caption rows {rows}: GEMM flops {gemm:.4e}, per-row terms x rows {expect:.4e}, ratio {gemm / expect:.4f}")
    assert abs(gemm / expect - 1) < 0.01


def test_per_context_attention_refuses_a_ragged_context_before_any_launch(cuda):
    from mj_video_amd import ops
    model = model_of("tiny", cuda)
    cfg, videos, prompts, index, ids, mask, first = case_tensors("tiny", "one", cuda)
    ctx = model.encode_video(videos[0], prompts[0], context_len=117)
    torch.cuda.synchronize()
    model.caption_attention = "per-context"
    try:
        ops.prof_enable(True)
        ops.prof_reset()
        with pytest.raises(ValueError, match=r"context 0 holds 117 tokens.*multiple of 64"):
            model.score_captions(ctx, ids, mask)
        assert not ops.prof_results(), "a refused call launched something"
    finally:
        ops.prof_enable(False)
        ops.prof_reset()
        model.caption_attention = "shared"
    assert torch.isfinite(model.score_captions(ctx, ids, mask).score).all()


def test_caption_matrix_with_shared_contexts(cuda):
    """harness.score_caption_matrix(context="shared") for 3 videos x 4 captions under the bound of
    test_score_caption_matrix_equals_single_forwards: per block of the packed rows rms(matrix - fp32 oracle) <= 2 x rms(single
    forwards - fp32 oracle) + ATOL_FLOOR; one video per call and blocks of videos: equal bits at these dims; context="video" is
    the call without the argument, bit for bit"""
    from mj_video_amd import harness, synth
    from mj_video_amd.chat_input import prepare_chat_input, video_prefix
    from oracle import ref_cpu
    from test_host_logic import StubTokenizer
    model = model_of("tiny", cuda)
    cfg = cu_.cfg_of("tiny")
    sd32 = {k: v.float() for k, v in synth.synth_state_dict(cfg, seed=0).items()}
    tok = StubTokenizer()
    videos = [synth.synth_pixel_values(31, v, t, 56) for v, t in enumerate((4, 3, 2))]
    captions = ["a cat walks over a red carpet", "two dogs", "the camera pans slowly over a harbour at dusk, boats", "x"]
    dv = [v.to(cuda) for v in videos]
    default = harness.score_caption_matrix(model, cfg, tok, dv, captions, {}, max_rows=5)
    assert torch.equal(harness.score_caption_matrix(model, cfg, tok, dv, captions, {}, max_rows=5, context="video"), default)
    shared_t = harness.score_caption_matrix(model, cfg, tok, dv, captions, {}, max_rows=5, context="shared")
    blocks = harness.score_caption_matrix(model, cfg, tok, dv, captions, {}, max_rows=5, videos_per_call=2, context="shared")
    assert torch.equal(shared_t, blocks), "shared contexts: blocks of videos and one video per call differ"
    one = harness.score_video_captions(model, cfg, tok, dv[1], captions, {}, context="shared")
    assert torch.equal(one, shared_t[1]), "one video alone scores as its row of the matrix"
    with pytest.raises(ValueError, match="context 'prefix' not in"):
        harness.score_caption_matrix(model, cfg, tok, dv, captions, {}, context="prefix")
    mat = shared_t.float().cpu().numpy()
    assert mat.shape == (3, 4, 34)
    singles, oracle, lens = np.zeros_like(mat), np.zeros_like(mat), []
    model.prefix_cache = False
    for v, pv in enumerate(videos):
        rows = []
        for j, c in enumerate(captions):
            ids, mask = prepare_chat_input(cfg, tok, pv, video_prefix(pv.shape[0]) + c, {}, device="cpu")
            rows.append(ids)
            model.forward(pv.to(cuda), ids.to(cuda), mask.to(cuda))
            singles[v, j] = model.last_packed34[0].float().cpu().numpy()
            ref = ref_cpu.reward_forward(sd32, cfg, pv.float(), ids, mask, synth.IMG_CONTEXT_ID, synth.PAD_ID)
            oracle[v, j] = np.concatenate([ref["score"].numpy().reshape(-1), ref["aspect_scores"].numpy().reshape(-1),
                                           ref["rewards"].float().numpy().reshape(-1)])
        lens.append(harness.shared_prefix_len(rows, synth.PAD_ID))
    model.prefix_cache = True
    print(f"shared prefix lengths of the three videos: {lens}")
    assert any(L % 64 for L in lens), "the shared contexts of this test must not all be whole tiles"
    nasp = model.num_aspects
    for name, sl in (("score", slice(0, 1)), ("aspect_scores", slice(1, 1 + nasp)), ("rewards", slice(1 + nasp, 34))):
        a, b = rms(mat[..., sl] - oracle[..., sl]), rms(singles[..., sl] - oracle[..., sl])
        print(f"matrix over shared contexts, {name}: rms(matrix - fp32 oracle) {a:.4e}, rms(single forwards - fp32 oracle) {b:.4e}")
        assert a <= 2 * b + ATOL_FLOOR, (name, a, b)
