"""mjv_attention_ctx_bf16 (include/mjv.h, ABI 7 additive): causal attention of few own rows per sequence over long, shared
key / value contexts - against the fp32 reference of tests/test_kernels_gpu.py on the concatenated [context | own] rows, against
the existing kernel with prefix_k / prefix_v, and its determinism / independence / refusal contracts."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_kernels_gpu import assert_close_bf16, attn_reference, rnd

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
D = 128


def attn_reference_rows(q, k, v, H, G, scale, mode):
    """``attn_reference`` of tests/test_kernels_gpu.py (causal) for ONE sequence whose queries are its LAST q.shape[0] rows: the
    same statements on those score rows only - a 28 872-key sequence's full score matrix is 3.3 GB per head.
    ``test_reference_rows_is_attn_reference`` holds the two to equal bits."""
    nq, L = q.shape[0], k.shape[0]
    out = torch.zeros(nq, H * D)
    masked = torch.arange(L)[None, :] > (L - nq + torch.arange(nq))[:, None]
    for h in range(H):
        qh = q[:, h * D:(h + 1) * D].float()
        kh = k[:, (h // G) * D:(h // G + 1) * D].float()
        vh = v[:, (h // G) * D:(h // G + 1) * D].float()
        sc = qh @ kh.t()
        if mode == 2:
            sc = sc * scale
        else:
            sc = (sc.to(BF).float() * scale).to(BF).float()
        sc = sc.masked_fill(masked, float("-inf"))
        p = torch.softmax(sc, -1).to(BF).float()
        out[:, h * D:(h + 1) * D] = p @ vh
    return out.to(BF)


def test_reference_rows_is_attn_reference():
    """(needs no GPU work, but lives with the tests it serves)"""
    for mode in (1, 2):
        L, nq, H, G = 300, 37, 4, 2
        q, k, v = rnd(L, H * D, seed=1), rnd(L, (H // G) * D, seed=2), rnd(L, (H // G) * D, seed=3)
        full = attn_reference(q, k, v, [L], H, G, D, True, D ** -0.5, mode)
        rows = attn_reference_rows(q[L - nq:], k, v, H, G, D ** -0.5, mode)
        # (a row's softmax does not depend on the other rows; the matmuls may block differently: a last-bit tolerance)
        assert_close_bf16(rows, full[L - nq:], 1, frac_exact=0.99, atol=1e-6, what="rows-only reference")


class Problem:
    """own rows / contexts of one launch, on the host (bf16) - and the fp32 reference per sequence"""

    def __init__(self, ctx_lens, own_lens, index, H, G, q_lens=None, seed=0):
        self.ctx_lens, self.own_lens, self.index, self.H, self.G = list(ctx_lens), list(own_lens), list(index), H, G
        self.q_lens = list(q_lens) if q_lens is not None else None
        KV = H // G
        n, nc = sum(own_lens), sum(ctx_lens)
        self.k, self.v = rnd(n, KV * D, seed=seed + 2), rnd(n, KV * D, seed=seed + 3)
        self.ck, self.cv = rnd(nc, KV * D, seed=seed + 4), rnd(nc, KV * D, seed=seed + 5)
        self.cu = np.concatenate([[0], np.cumsum(own_lens)]).astype(np.int32)
        self.cu_ctx = np.concatenate([[0], np.cumsum(ctx_lens)]).astype(np.int32)
        ql = self.q_lens if self.q_lens is not None else self.own_lens
        self.cu_q = np.concatenate([[0], np.cumsum(ql)]).astype(np.int32)
        self.q = rnd(int(self.cu_q[-1]), H * D, seed=seed + 1)

    def reference(self, mode, seqs=None):
        """fp32 reference rows (bf16) of the queries, sequence by sequence on [context | own]"""
        out = torch.zeros(int(self.cu_q[-1]), self.H * D, dtype=BF)
        for s in (range(len(self.own_lens)) if seqs is None else seqs):
            c = self.index[s]
            c0, c1, s0, s1 = self.cu_ctx[c], self.cu_ctx[c + 1], self.cu[s], self.cu[s + 1]
            kk = torch.cat([self.ck[c0:c1], self.k[s0:s1]])
            vv = torch.cat([self.cv[c0:c1], self.v[s0:s1]])
            q0, q1 = self.cu_q[s], self.cu_q[s + 1]
            out[q0:q1] = attn_reference_rows(self.q[q0:q1], kk, vv, self.H, self.G, D ** -0.5, mode)
        return out

    def run(self, dev, mode, prefill=None):
        from mj_video_amd import ops
        plan = ops.AttnCtxPlan(self.cu, self.index, self.cu_ctx, self.H, self.G, D, dev,
                               cu_seqlens_q=self.cu_q if self.q_lens is not None else None)
        ws = torch.empty(plan.workspace_bytes, dtype=torch.uint8, device=dev)
        out = torch.empty(int(self.cu_q[-1]) + 3, self.H * D, dtype=BF, device=dev)   # (+ 3 rows nobody may touch)
        out.fill_(float("nan") if prefill is None else prefill)
        ops.attention_ctx(self.q.to(dev), self.k.to(dev), self.v.to(dev), out, self.ck.to(dev), self.cv.to(dev), plan,
                          D ** -0.5, mode, ws)
        torch.cuda.synchronize()
        return out.cpu()


def mixed_lengths(n, seed):
    """own lengths from 1 to 200, both ends present"""
    g = np.random.default_rng(seed)
    lens = g.integers(1, 201, size=n).tolist()
    lens[0] = 1
    if n > 1:
        lens[-1] = 200
    return lens


def check_against_fp32(out, ref, nq, what):
    got, want = out[:nq].float(), ref.float()
    assert torch.isfinite(got).all(), f"{what}: NaN / inf left in query rows"
    rel = ((got - want).norm() / want.norm()).item()
    print(f"{what}: relative L2 {rel:.3e}, max abs {(got - want).abs().max().item():.3e}")
    assert rel < 4e-3, f"{what}: relative L2 error {rel:.3e}"
    assert_close_bf16(out[:nq], ref, 2, atol=0.02, what=what)
    assert torch.isnan(out[nq:].float()).all(), f"{what}: rows behind the queries were written"


# (context lengths, sequences, context_index pattern, H, G, suffix queries)
SHAPES = [
    ([64], 1, None, 16, 2, False),
    ([64], 5, None, 4, 2, False),
    ([2112], 1, None, 16, 2, False),
    ([2112], 2, None, 16, 2, False),
    ([2112], 5, None, 16, 2, True),
    ([2112], 48, None, 16, 2, False),
    ([2112], 48, None, 4, 2, True),
    ([28672], 2, None, 4, 2, False),
    ([28672], 5, None, 16, 2, False),
    ([2112, 576], 5, [0, 1, 0, 1, 1], 16, 2, False),
    ([576, 2112, 64], 48, "interleave", 4, 2, True),
    ([2112, 64, 1536], 5, [2, 0, 1, 2, 0], 16, 2, True),
]


def make_problem(ctx_lens, n, index, H, G, suffix, seed=10):
    own = mixed_lengths(n, seed)
    if index is None:
        index = [0] * n
    elif index == "interleave":
        index = [i % len(ctx_lens) for i in range(n)]
    q_lens = None
    if suffix:   # the last few own rows only (1 .. 7, never more than the sequence has)
        q_lens = [min(L, 1 + (i * 3) % 7) for i, L in enumerate(own)]
    return Problem(ctx_lens, own, index, H, G, q_lens, seed=seed)


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("ctx_lens,n,index,H,G,suffix", SHAPES)
def test_ctx_attention_vs_fp32(cuda, ctx_lens, n, index, H, G, suffix, mode):
    """(1) of the issue: same error model as test_attention (P rounded before vs after normalisation), and fp32 partials merged
    in fp32 by exact powers of two add no rounding point: the same bounds."""
    p = make_problem(ctx_lens, n, index, H, G, suffix)
    out = p.run(cuda, mode)
    check_against_fp32(out, p.reference(mode), int(p.cu_q[-1]), f"ctx{ctx_lens} n={n} H={H} suffix={suffix} mode={mode}")


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("ctx_len,n,H,suffix", [(64, 5, 4, False), (2112, 1, 16, False), (2112, 5, 16, True), (2112, 48, 16, False),
                                                (28672, 2, 4, False)])
def test_ctx_attention_vs_prefix_kernel(cuda, ctx_len, n, H, suffix, mode):
    """(2): the single-context problems through ops.attention with prefix_k / prefix_v - both kernels are held to fp32 elsewhere;
    this catches a mistake in the test's own [context | own] layout.  Relative L2 between the two < 4e-3."""
    from mj_video_amd import ops
    p = make_problem([ctx_len], n, None, H, 2, suffix)
    out = p.run(cuda, mode)
    nq = int(p.cu_q[-1])
    old = torch.empty(nq, H * D, dtype=BF, device=cuda)
    kw = {}
    if suffix:
        kw = dict(cu_seqlens_q=torch.from_numpy(p.cu_q).to(cuda), max_seqlen_q=max(p.q_lens))
    ops.attention(p.q.to(cuda), p.k.to(cuda), p.v.to(cuda), old, torch.from_numpy(p.cu).to(cuda), max(p.own_lens), H, 2, D, True,
                  D ** -0.5, mode, prefix_k=p.ck.to(cuda), prefix_v=p.cv.to(cuda), **kw)
    torch.cuda.synchronize()
    a, b = out[:nq].float(), old.float().cpu()
    rel = ((a - b).norm() / b.norm()).item()
    print(f"ctx {ctx_len} n={n}: relative L2 between the two kernels {rel:.3e}")
    assert rel < 4e-3


def test_ctx_attention_equal_bits_and_independence(cuda):
    """two launches give equal bits; a sequence's rows keep their bits when sequences of ANOTHER context join the launch"""
    own = mixed_lengths(7, 3)
    alone = Problem([2112], own, [0] * 7, 16, 2, seed=20)
    a1, a2 = alone.run(cuda, 2), alone.run(cuda, 2)
    nq = int(alone.cu_q[-1])
    assert torch.equal(a1[:nq].view(torch.int16), a2[:nq].view(torch.int16))
    # the same seven sequences interleaved with nine of a second context (their own data: other seeds)
    extra = mixed_lengths(9, 4)
    both = Problem([2112, 576], own + extra, [0] * 7 + [1] * 9, 16, 2, seed=20)
    order = [0, 7, 8, 1, 9, 2, 3, 10, 11, 12, 4, 13, 5, 14, 6, 15]
    mixed = Problem([2112, 576], [both.own_lens[i] for i in order], [both.index[i] for i in order], 16, 2, seed=99)
    other = Problem([576], extra, [0] * 9, 16, 2, seed=40)
    mixed.ck = torch.cat([alone.ck, other.ck])
    mixed.cv = torch.cat([alone.cv, other.cv])
    rows = {"q": [], "k": [], "v": []}
    for i in order:
        src, j = (alone, i) if i < 7 else (other, i - 7)
        for nm in rows:
            rows[nm].append(getattr(src, nm)[src.cu[j]:src.cu[j + 1]])
    mixed.q, mixed.k, mixed.v = (torch.cat(rows[nm]) for nm in ("q", "k", "v"))
    m = mixed.run(cuda, 2)
    for pos, i in enumerate(order):
        if i < 7:
            got = m[mixed.cu[pos]:mixed.cu[pos + 1]]
            want = a1[alone.cu[i]:alone.cu[i + 1]]
            assert torch.equal(got.view(torch.int16), want.view(torch.int16)), f"sequence {i} changed bits next to another context"


def test_ctx_attention_refusals(cuda):
    """every refusal is decided on the host side of the C entry, before any launch"""
    from mj_video_amd import _lib, ops
    p = make_problem([128], 3, None, 4, 2, False)
    plan = ops.AttnCtxPlan(p.cu, p.index, p.cu_ctx, 4, 2, D, cuda)
    ws = torch.empty(plan.workspace_bytes, dtype=torch.uint8, device=cuda)
    out = torch.zeros(int(p.cu[-1]), 4 * D, dtype=BF, device=cuda)
    t = [x.to(cuda) for x in (p.q, p.k, p.v)] + [out, p.ck.to(cuda), p.cv.to(cuda)]
    with pytest.raises(_lib.MjvLibraryError, match=r"\(-3\).*causal"):
        ops.attention_ctx(*t, plan, D ** -0.5, 2, ws, causal=False)
    with pytest.raises(_lib.MjvLibraryError, match=r"\(-1\).*workspace"):
        ops.attention_ctx(*t, plan, D ** -0.5, 2, None)
    with pytest.raises(_lib.MjvLibraryError, match=r"\(-1\).*workspace"):
        ops.attention_ctx(*t, plan, D ** -0.5, 2, ws[:plan.workspace_bytes - 16])
    with pytest.raises(_lib.MjvLibraryError, match=r"\(-1\).*score_round_mode"):
        ops.attention_ctx(*t, plan, D ** -0.5, 0, ws)
    with pytest.raises(_lib.MjvLibraryError, match=r"\(-1\).*multiple of 64"):
        ops.AttnCtxPlan(p.cu, p.index, np.array([0, 100], dtype=np.int32), 4, 2, D, cuda)
    with pytest.raises(_lib.MjvLibraryError, match=r"\(-1\).*names context"):
        ops.AttnCtxPlan(p.cu, [0, 1, 0], p.cu_ctx, 4, 2, D, cuda)
    with pytest.raises(_lib.MjvLibraryError, match=r"\(-3\).*head_dim 64"):
        ops.AttnCtxPlan(p.cu, p.index, p.cu_ctx, 4, 2, 64, cuda)
    # a short plan: the entry knows the size the index arrays need
    d = plan.desc()
    d.Q = d.K = d.V = d.O = d.ctx_k = d.ctx_v = out.data_ptr()
    d.ldq = d.ldk = d.ldv = d.ldo = d.ld_ctx_k = d.ld_ctx_v = 4 * D
    d.scale, d.score_round_mode = D ** -0.5, 2
    d.plan, d.plan_ints = plan.plan.data_ptr(), plan.plan_ints - 1
    d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel()
    lib = _lib.load_library()
    assert lib.mjv_attention_ctx_bf16(C.byref(d), None) == -1 and b"plan" in lib.mjv_last_error()
    torch.cuda.synchronize()
    assert not out.float().abs().sum().item(), "a refused call wrote output"


# ------------------------------------------------------------------------------------------------------------------------
# model.encode_video / model.score_captions end to end
import captions_util as cu_  # noqa: E402
from test_e2e_gpu import ATOL_FLOOR  # noqa: E402
from util import FIELDS, build_hip_model  # noqa: E402

_MODELS = {}
RMS_FIELDS = ("score", "aspect_scores", "rewards", "criteria_gating_output", "aspect_gating_output")
HIDDEN_FIELDS = ("hidden_state", "prompt_embedding")


def model_of(dims, dev):
    """one model per dims for the whole module (synthetic weights, seed 0: the fixtures' checkpoint)"""
    from mj_video_amd import synth
    if dims not in _MODELS:
        cfg = cu_.cfg_of(dims)
        sd = synth.synth_state_dict(cfg, seed=0, lm_head=False)
        sd["model.language_model.output.weight"] = torch.zeros(1, dtype=torch.bfloat16).expand(
            cfg.llm_config.vocab_size, cfg.llm_config.hidden_size)
        _MODELS[dims] = build_hip_model(cfg, sd, dev)
    m = _MODELS[dims]
    m.caption_attention, m.prefix_cache, m.trim_last_layer = "shared", True, True
    m.set_ffn_format("bf16")
    return m


def case_tensors(dims, case, dev):
    from mj_video_amd import synth
    cfg, videos, prompts, index = cu_.CASES[case](dims)
    ids, mask = synth.pad_batch(prompts)
    first = [int(np.flatnonzero(index == v)[0]) for v in range(len(videos))]
    return cfg, [v.to(dev) for v in videos], prompts, index, ids.to(dev), mask.to(dev), first


def encode_all(model, videos, prompts, first):
    return [model.encode_video(v, prompts[first[i]]) for i, v in enumerate(videos)]


def rms(a):
    return float(np.sqrt(np.mean(np.square(np.asarray(a, dtype=np.float64)))))


def rel_l2(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


@pytest.mark.parametrize("mode", ["shared", "per-context"])
@pytest.mark.parametrize("case", ["one", "multi"])
@pytest.mark.parametrize("dims", ["tiny", "2b"])
def test_score_captions_vs_oracle_and_forward(cuda, dims, case, mode):
    """(3) / (4) of the issue.  Reference: the fp32 oracle on the full prompts (tests/golden/captions_*.npz); second witness:
    ``forward`` on the same full prompts with prefix_cache = False.  Both HIP results are bf16 evaluations of one function that
    differ in fp32 summation order and GEMM tile choice, so per field rms(score_captions - oracle) <= 2 x rms(forward - oracle) +
    ATOL_FLOOR; the two hidden rows: relative L2 to the oracle no more than 2 x forward's own.
    Measured on an MI355X (docs/captions.md holds every figure): rms(score_captions) / rms(forward) between 0.59 and 1.48 over every
    field, case and mode; 2B dims, one video: score 5.06e-2 against 6.12e-2, 32 of 66 pairs decisive, none flipped."""
    model = model_of(dims, cuda)
    cfg, videos, prompts, index, ids, mask, first = case_tensors(dims, case, cuda)
    f32, bf16 = cu_.load_golden_captions(dims, case)
    ctxs = encode_all(model, videos, prompts, first)
    model.caption_attention = mode
    out = model.score_captions(ctxs, ids, mask, context_index=torch.from_numpy(index))
    packed = model.last_packed34.float().cpu().numpy()
    model.prefix_cache = False
    fw = model.forward(torch.cat([videos[int(c)] for c in index]), ids, mask)
    torch.cuda.synchronize()
    got = {f: getattr(out, f).float().cpu().numpy() for f in FIELDS}
    wit = {f: getattr(fw, f).float().cpu().numpy() for f in FIELDS}
    for f in FIELDS:
        assert getattr(out, f).dtype == getattr(fw, f).dtype and getattr(out, f).shape == getattr(fw, f).shape, f
    assert np.array_equal(packed[:, 0], got["score"]) and packed.shape == (len(prompts), 34)
    failures = []
    for f in RMS_FIELDS:
        a, b = rms(got[f] - f32[f]), rms(wit[f] - f32[f])
        print(f"{dims} {case} {mode} {f}: rms(score_captions - fp32 oracle) {a:.4e}, rms(forward - fp32 oracle) {b:.4e}")
        if not a <= 2 * b + ATOL_FLOOR:
            failures.append((f, a, b))
    for f in HIDDEN_FIELDS:
        a, b = rel_l2(got[f], f32[f]), rel_l2(wit[f], f32[f])
        print(f"{dims} {case} {mode} {f}: relative L2 to the fp32 oracle {a:.4e} (score_captions), {b:.4e} (forward)")
        if not a <= 2 * b:
            failures.append((f, a, b))
    assert not failures, failures
    if case == "one":
        # order: every pair of captions whose fp32-oracle scores differ by more than 6 x rms(bf16 oracle - fp32 oracle)
        thr = 6 * rms(bf16["score"] - f32["score"])
        s32, s = f32["score"], got["score"]
        n = len(s32)
        pairs = [(i, j) for i in range(n) for j in range(i + 1, n) if abs(s32[i] - s32[j]) > thr]
        print(f"{dims} {mode}: {len(pairs)} of {n * (n - 1) // 2} pairs decisive at {thr:.4f}")
        assert len(pairs) >= 24, f"only {len(pairs)} decisive pairs: the order check would be vacuous"
        flips = [(i, j) for i, j in pairs if (s32[i] > s32[j]) != (s[i] > s[j])]
        assert not flips, f"score_captions orders {flips} against the fp32 oracle"


def test_score_captions_leaves_the_shared_work_out(cuda):
    """(5): no ViT and no context rows in a score_captions call - the profiler sees no attn_d64 / patchify launch, and the GEMM
    flops are those of the caption rows: bench.py's per-token terms (executed_tflop_per_video: every Linear of 23 layers, the
    last layer's k | v projection) x caption rows, within 1 % (the last layer's tail / selected rows and the gating MLPs are
    the rest); encode_video runs the ViT exactly once."""
    from mj_video_amd import ops
    dims = "2b"
    model = model_of(dims, cuda)
    cfg, videos, prompts, index, ids, mask, first = case_tensors(dims, "one", cuda)
    l = cfg.llm_config
    try:
        ops.prof_enable(True)
        ops.prof_reset()
        ctxs = encode_all(model, videos, prompts, first)
        enc = ops.prof_results()
        ops.prof_reset()
        model.score_captions(ctxs, ids, mask)
        cap = ops.prof_results()
    finally:
        ops.prof_enable(False)
        ops.prof_reset()
    n_vit = cfg.vision_config.num_hidden_layers
    assert enc["patchify"]["launches"] == 1 and enc["attn_d64"]["launches"] == n_vit, "encode_video runs the ViT exactly once"
    assert "attn_d64" not in cap and "patchify" not in cap and "attn_d128_causal" not in cap, sorted(cap)
    assert cap["attn_ctx_d128"]["launches"] == l.num_hidden_layers
    rows = sum(p.shape[1] - ctxs[0].P for p in prompts)
    h, ff = l.hidden_size, l.intermediate_size
    hd = h // l.num_attention_heads
    qkv_out, kv_out = (l.num_attention_heads + 2 * l.num_key_value_heads) * hd, 2 * l.num_key_value_heads * hd
    per_tok = 2.0 * (h * qkv_out + l.num_attention_heads * hd * h + 3 * h * ff)
    expect = ((l.num_hidden_layers - 1) * per_tok + 2.0 * h * kv_out) * rows
    gemm = sum(v["flops"] for k, v in cap.items() if k.startswith("gemm"))
    print(f"caption rows {rows}: GEMM flops {gemm:.4e}, per-row terms x rows {expect:.4e}, ratio {gemm / expect:.4f}")
    assert abs(gemm / expect - 1) < 0.01
    # attention: 4 D sum(queries x keys each sees) per q-head
    pairs = 0.0
    for p in prompts:
        L = p.shape[1] - ctxs[0].P
        pairs += (l.num_hidden_layers - 1) * (L * ctxs[0].P + L * (L + 1) / 2) + (5 * ctxs[0].P + sum(L - 4 + i for i in range(5)))
    want = 4.0 * hd * pairs * l.num_attention_heads
    assert abs(cap["attn_ctx_d128"]["flops"] / want - 1) < 1e-6, (cap["attn_ctx_d128"]["flops"], want)


def test_score_captions_refusals_and_lifetime(cuda):
    """(6): every ValueError of the interface; a context survives forwards in between; prefix_cache_hits / _prefix untouched by
    the new methods; stale contexts (new weights, other numerics) are refused, never rebuilt."""
    from mj_video_amd import synth
    from mj_video_amd.modeling import VideoContext
    dims = "tiny"
    model = model_of(dims, cuda)
    cfg, videos, prompts, index, ids, mask, first = case_tensors(dims, "multi", cuda)
    idx = torch.from_numpy(index)
    hits, pref = model.prefix_cache_hits, model._prefix
    ctxs = encode_all(model, videos, prompts, first)
    assert all(isinstance(c, VideoContext) and c.P % 64 == 0 and c.P > 0 for c in ctxs)
    lc = cfg.llm_config
    assert ctxs[0].nbytes == (2 * ctxs[0].P * lc.num_key_value_heads * 128 * lc.num_hidden_layers + ctxs[0].img_tail.numel()) * 2
    base = model.score_captions(ctxs, ids, mask, context_index=idx)
    assert model.prefix_cache_hits == hits and model._prefix is pref
    # forwards in between (other prompts, the prefix cache at work) leave the contexts alone
    model.forward(torch.cat([videos[int(c)] for c in index]), ids, mask)
    again = model.score_captions(ctxs, ids, mask, context_index=idx)
    for f in FIELDS:
        assert torch.equal(getattr(base, f), getattr(again, f)), f
    P = ctxs[0].P

    def refused(match, ids_=ids, mask_=mask, ctxs_=ctxs, idx_=idx):
        with pytest.raises(ValueError, match=match):
            model.score_captions(ctxs_, ids_, mask_, context_index=idx_)

    bad = ids.clone()
    bad[4, 7] += 1
    refused(r"row 4: its first \d+ token ids differ", ids_=bad)
    m2 = mask.clone()
    m2[2, P - 1] = 0
    refused(r"row 2: masked column", mask_=m2)
    refused(r"row 1: \d+ <IMG_CONTEXT> tokens", idx_=torch.tensor([0, 0, 2] + list(index[3:])))   # (row 1's ids ARE context 0's up to P)
    # a row that ends inside its context: every column behind P padded, the gating pattern in front of P (its context is
    # given those ids, so that THIS check is the one that speaks)
    short = ids[5:6].clone()
    short[0, P:] = synth.PAD_ID
    short[0, P - 6:P - 1] = torch.tensor(synth.GATING_PATTERN)
    import copy
    c5 = copy.copy(ctxs[int(index[5])])
    c5.ids = short[0, :P].cpu().numpy()
    refused(r"row 0: reward row \d+ / gating row \d+ lies inside its context", ids_=short, mask_=mask[5:6], ctxs_=[c5], idx_=None)
    refused(r"row 3: context_index 3 out of range", idx_=torch.tensor([0, 1, 2, 3] + list(index[4:])))
    model.attention_scores = "eager" if model.attention_scores == "flash" else "flash"
    try:
        refused(r"context 0 was built under other settings")
    finally:
        model.attention_scores = "eager" if model.attention_scores == "flash" else "flash"
    model.set_ffn_format("mxfp8")
    try:
        refused(r"context 0 was built under other settings")
        # (the presets work: context and caption pass under the same format)
        c8 = encode_all(model, videos, prompts, first)
        o8 = model.score_captions(c8, ids, mask, context_index=idx)
        assert torch.isfinite(o8.score).all() and torch.isfinite(o8.rewards.float()).all()
    finally:
        model.set_ffn_format("bf16")
    other = copy.copy(ctxs[1])
    other.device = torch.device("cuda:1")
    refused(r"context 1 lives on cuda:1", ctxs_=[ctxs[0], other, ctxs[2]])
    model.score_captions(ctxs, ids, mask, context_index=idx)      # still good
    sd = model.state_dict()
    model.load_state_dict(sd, strict=True)                        # new weights (same values: the versions moved)
    refused(r"context 0 was built under other settings")
    fresh = encode_all(model, videos, prompts, first)
    after = model.score_captions(fresh, ids, mask, context_index=idx)
    for f in FIELDS:
        assert torch.equal(getattr(base, f), getattr(after, f)), f


def test_context_on_another_stream_waits_for_its_event(cuda):
    """(6), the two-thread pattern of test_two_threads_two_streams_score_bitwise, with the wait given something to do: in every
    round the contexts are encoded on the MAIN stream behind a long-running kernel and, with no synchronise in between, two
    threads score caption sets of them, each with its own model instance on its own stream.  The context rows do not exist yet
    when the side streams are handed their work: only the ready-event orders them.  Every round encodes OTHER videos than the
    round before (a stale block of the caching allocator cannot stand in for the rows) and must equal, bit for bit, what the
    same calls give on one stream."""
    import threading
    from mj_video_amd import synth
    cfg = cu_.cfg_of("tiny")
    sd = synth.synth_state_dict(cfg, seed=0)
    models = [build_hip_model(cfg, sd, cuda) for _ in range(2)]
    rounds = []
    for rnd_ in range(3):
        per_thread = []
        for i, case in enumerate(("one", "multi")):
            _, videos, prompts, index, ids, mask, first = case_tensors("tiny", case, cuda)
            videos = [synth.synth_pixel_values(200 + 10 * rnd_ + i, v, vid.shape[0], 56).to(cuda) for v, vid in enumerate(videos)]
            per_thread.append((videos, prompts, first, ids, mask, torch.from_numpy(index)))
        rounds.append(per_thread)
    expect = []
    for per_thread in rounds:      # single-stream results, everything synchronised
        row = []
        for i, (videos, prompts, first, ids, mask, index) in enumerate(per_thread):
            row.append(models[i].score_captions(encode_all(models[i], videos, prompts, first), ids, mask, context_index=index))
            torch.cuda.synchronize()
        expect.append(row)
    assert not torch.equal(expect[0][0].score, expect[1][0].score), "the rounds must differ for the check to see stale rows"
    for rnd_, per_thread in enumerate(rounds):
        got, errs = [None, None], []
        torch.cuda.synchronize()
        torch.cuda._sleep(400_000_000)       # (a few hundred ms of the main stream: the encodes below queue behind it)
        ctxs = [encode_all(models[i], t[0], t[1], t[2]) for i, t in enumerate(per_thread)]
        assert not ctxs[0][0].ready.query(), "the context rows must still be pending when the side streams start"

        def work(i):
            try:
                st = torch.cuda.Stream(device=cuda)
                with torch.cuda.stream(st):
                    got[i] = models[i].score_captions(ctxs[i], per_thread[i][3], per_thread[i][4], context_index=per_thread[i][5])
                st.synchronize()
            except Exception as e:   # surfaced below
                errs.append(e)

        ts = [threading.Thread(target=work, args=(i,)) for i in range(2)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        assert not errs, errs
        for i in range(2):
            for f in FIELDS:
                assert torch.equal(getattr(got[i], f), getattr(expect[rnd_][i], f)), (rnd_, i, f)
        torch.cuda.synchronize()
        del ctxs


def test_context_refused_once_dynamic_ntk_has_moved_the_rotary_base(cuda):
    """(6), the last ValueError of the interface: a context's keys are rotated with the base in force when it was encoded.  With
    dynamic-NTK scaling the reference replaces its inv_freq FOR GOOD the first time a (padded) sequence longer than
    max_position_embeddings reaches the tower (modeling_internlm2.py:204-229; ``_rope_next_state``), and every later call, short
    ones included, rotates with the rescaled base.  Tiny dims, max_position_embeddings = 200, prompts of 123 ... 282 columns:
    * a context encoded at 123 columns serves batches up to 200 columns wide (nothing moved);
    * a batch 282 columns wide WOULD move the base: refused before anything advances (the next short call still scores, bits
      unchanged);
    * a ``forward`` on that wide batch moves the base; the old context is refused from then on, for every width;
    * a freshly encoded context scores, and agrees with ``forward`` under the same (moved) state: both lie 6.6e-3 (relative L2
      of the hidden rows, docs/captions.md, tiny dims) from the fp32 function, so within 2 x that of one another - 1.5e-2 with
      margin for another box's summation order."""
    from mj_video_amd import configuration as C, synth
    cd = C.tiny_config_dict(56)
    cd["llm_config"]["max_position_embeddings"] = 200
    cd["llm_config"]["rope_scaling"] = dict(type="dynamic", factor=2.0)
    cfg = C.InternVLChatRewardModelingConfig(**cd, **C.mjvideo_head_kwargs())
    model = build_hip_model(cfg, synth.synth_state_dict(cfg, seed=0), cuda)
    _, videos, prompts, _ = cu_.one_case("tiny")
    px = videos[0].to(cuda)
    widths = [p.shape[1] for p in prompts]
    assert widths[0] == 123 and widths[-1] == 282
    short = [p for p in prompts if p.shape[1] <= 200]
    assert len(short) >= 6 and max(p.shape[1] for p in short) > 150
    ids_s, mask_s = (t.to(cuda) for t in synth.pad_batch(short))
    ids_w, mask_w = (t.to(cuda) for t in synth.pad_batch(prompts))
    theta = float(cfg.llm_config.rope_theta)
    ctx = model.encode_video(px, prompts[0])
    assert model._rope_state == dict(cached=200, base=theta)
    base = model.score_captions(ctx, ids_s, mask_s)                      # wider than the encode, inside max_position_embeddings
    assert model._rope_state == dict(cached=200, base=theta)
    with pytest.raises(ValueError, match="context 0 was built under other settings"):
        model.score_captions(ctx, ids_w, mask_w)                         # this width would move the base
    assert model._rope_state == dict(cached=200, base=theta), "a refused call must not advance the rotary state"
    again = model.score_captions(ctx, ids_s, mask_s)
    for f in FIELDS:
        assert torch.equal(getattr(base, f), getattr(again, f)), f
    model.prefix_cache = False
    model.forward(px.repeat(len(prompts), 1, 1, 1), ids_w, mask_w)       # the base moves for good
    assert model._rope_state["cached"] == 282 and model._rope_state["base"] > theta
    for ids_, mask_ in ((ids_s, mask_s), (ids_w, mask_w), (ids_s[:1, :widths[0]].contiguous(), None)):
        with pytest.raises(ValueError, match="context 0 was built under other settings"):
            model.score_captions(ctx, ids_, mask_)
    fresh = model.encode_video(px, prompts[0])
    for ids_, mask_, n in ((ids_s, mask_s, len(short)), (ids_w, mask_w, len(prompts))):
        out = model.score_captions(fresh, ids_, mask_)
        fw = model.forward(px.repeat(n, 1, 1, 1), ids_, mask_)
        for f in ("hidden_state", "prompt_embedding"):
            d = rel_l2(getattr(out, f).float().cpu().numpy(), getattr(fw, f).float().cpu().numpy())
            print(f"moved base, {n} captions, {f}: relative L2 score_captions - forward {d:.4e}")
            assert d <= 1.5e-2, (f, d)
    # and the moved base is really in the fresh context: its keys differ from the old one's
    assert not torch.equal(fresh.k[0], ctx.k[0])


def test_score_caption_matrix_equals_single_forwards(cuda):
    """(7): harness.score_caption_matrix for 3 videos x 4 captions against twelve single scores through ``forward``, in
    [V, M, 34] order, with the bound of (4): per block of the packed rows (score | aspect scores | rewards)
    rms(matrix - fp32 oracle) <= 2 x rms(single forwards - fp32 oracle) + ATOL_FLOOR (the oracle at tiny dims runs here)."""
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
    mat = harness.score_caption_matrix(model, cfg, tok, [v.to(cuda) for v in videos], captions, {}, max_rows=5).float().cpu().numpy()
    assert mat.shape == (3, 4, 34)
    one = harness.score_video_captions(model, cfg, tok, videos[1].to(cuda), captions, {}).float().cpu().numpy()
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
        a, b = rms(mat[..., sl] - oracle[..., sl]), rms(singles[..., sl] - oracle[..., sl])
        print(f"matrix {name}: rms(matrix - fp32 oracle) {a:.4e}, rms(single forwards - fp32 oracle) {b:.4e}")
        assert a <= 2 * b + ATOL_FLOOR, (name, a, b)
    assert np.array_equal(one, mat[1]), "one video alone scores as its row of the matrix"
