"""mjv_attention_ctx_seg_bf16 (include/mjv.h, mjv_attn_ctx_segments): contexts that are concatenations of row ranges of several
tensors, shared between contexts - against the fp32 reference of tests/test_captions_gpu.py on the concatenated keys and against
the same keys as ONE contiguous any-length context through the existing entry; equal bits where the host plans' pieces
coincide, run to run, alone and in company; rows behind a use's length are never read; plain launches keep their bits."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_captions_gpu import BF, D, Problem, check_against_fp32, make_problem
from test_context_any_length_host import Plan
from test_kernels_gpu import rnd

pytestmark = pytest.mark.gpu

OWN = [1, 17, 70]
GEOMS = [(8, 8), (4, 1), (16, 8)]
TWO = [("A", 100), ("B", 37)]
THREE = [("A", 64), ("B", 1), ("C", 200)]
CUT = [("A", 1056), ("B", 1000), ("C", 56)]


def bits(t):
    return t.contiguous().view(torch.int16)


class SegProblem(Problem):
    """a ``Problem`` whose contexts are lists of (tensor name, use length): the tensors hold random rows (``extra`` more than the
    longest use reads), ``ck`` / ``cv`` are the concatenated keys / values the reference and the plain launch see"""

    def __init__(self, ctxs, own_lens, index, H, G, q_lens=None, seed=0, extra=0):
        super().__init__([sum(n for _, n in c) for c in ctxs], own_lens, index, H, G, q_lens, seed=seed)
        self.ctxs = [list(c) for c in ctxs]
        rows = {}
        for c in ctxs:
            for name, n in c:
                rows[name] = max(rows.get(name, 0), n)
        self.names = sorted(rows)
        KV = H // G
        self.tk = {nm: rnd(rows[nm] + extra, KV * D, seed=seed + 100 + 2 * i) for i, nm in enumerate(self.names)}
        self.tv = {nm: rnd(rows[nm] + extra, KV * D, seed=seed + 101 + 2 * i) for i, nm in enumerate(self.names)}
        self.concat()

    def concat(self):
        self.ck = torch.cat([self.tk[nm][:n] for c in self.ctxs for nm, n in c])
        self.cv = torch.cat([self.tv[nm][:n] for c in self.ctxs for nm, n in c])

    def segments(self):
        return [[(self.names.index(nm), n) for nm, n in c] for c in self.ctxs]

    def plan(self, dev, segmented=True):
        from mj_video_amd import ops
        return ops.AttnCtxPlan(self.cu, self.index, self.cu_ctx, self.H, self.G, D, dev, any_length=True,
                               cu_seqlens_q=self.cu_q if self.q_lens is not None else None,
                               segments=self.segments() if segmented else None, n_tensors=len(self.names) if segmented else None)

    def run(self, dev, mode, segmented=True, tk=None, tv=None):
        """segmented: the tensors where they lie; else ONE packed any-length buffer through the existing entry"""
        from mj_video_amd import ops
        plan = self.plan(dev, segmented)
        ws = torch.empty(plan.workspace_bytes, dtype=torch.uint8, device=dev)
        out = torch.full((int(self.cu_q[-1]) + 3, self.H * D), float("nan"), dtype=BF, device=dev)
        if segmented:
            tk, tv = tk or self.tk, tv or self.tv
            ck, cv = [tk[nm].to(dev) for nm in self.names], [tv[nm].to(dev) for nm in self.names]
        else:
            ck, cv = self.ck.to(dev), self.cv.to(dev)
        ops.attention_ctx(self.q.to(dev), self.k.to(dev), self.v.to(dev), out, ck, cv, plan, D ** -0.5, mode, ws,
                          segments=self.segments() if segmented else None)
        torch.cuda.synchronize()
        return out.cpu()


CASES = [(TWO, OWN, None), (TWO, OWN, [1, 3, 7]), (THREE, OWN, None), (THREE, OWN, [1, 17, 2]), (CUT, [1], None), (CUT, [9], [1])]


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("H,G", GEOMS)
@pytest.mark.parametrize("ctx,own,q_lens", CASES, ids=["100+37", "100+37-suffix", "64+1+200", "64+1+200-suffix", "cut", "cut-suffix"])
def test_segments_vs_fp32_and_vs_one_contiguous_context(cuda, ctx, own, q_lens, H, G, mode):
    p = SegProblem([ctx], own, [0] * len(own), H, G, q_lens, seed=30)
    nq = int(p.cu_q[-1])
    ref = p.reference(mode)
    what = f"{ctx} own={own} q={q_lens} H={H} G={G} mode={mode}"
    seg = p.run(cuda, mode)
    check_against_fp32(seg, ref, nq, "segments " + what)
    plain = p.run(cuda, mode, segmented=False)
    check_against_fp32(plain, ref, nq, "contiguous " + what)
    assert torch.equal(bits(seg[:nq]), bits(p.run(cuda, mode)[:nq])), "equal bits run to run"


@pytest.mark.parametrize("mode", [1, 2])
def test_equal_bits_where_the_segment_boundaries_are_piece_boundaries(cuda, mode):
    """2 176 keys under one query and one kv head are cut into 17 pieces of 128 keys; segments of 1 280 + 896 keys end on
    those boundaries, so both launches run the same pieces in the same order: the same bits"""
    p = SegProblem([[("A", 1280), ("B", 896)]], [1], [0], 8, 8, seed=31)
    a, b = Plan(p.plan(cuda).plan.cpu().numpy(), 8), Plan(p.plan(cuda, False).plan.cpu().numpy(), 8)
    assert a.n_parts == b.n_parts == 18 and np.array_equal(a.tiles, b.tiles)
    pa, pb = a.pieces(0), b.pieces(0)
    start = np.where(pa[:, 3] == 1, 1280, 0)      # a part's keys are relative to its tensor
    assert np.array_equal(pa[:, 1] + start, pb[:, 1]) and np.array_equal(pa[:, 2] + start, pb[:, 2])
    assert pa[:10, 3].tolist() == [0] * 10 and pa[10:, 3].tolist() == [1] * 7
    seg, plain = p.run(cuda, mode), p.run(cuda, mode, segmented=False)
    check_against_fp32(seg, p.reference(mode), 1, f"1280+896 mode={mode}")
    assert torch.equal(bits(seg[:1]), bits(plain[:1]))


@pytest.mark.parametrize("mode", [1, 2])
def test_contexts_that_share_tensors_keep_their_bits_in_company(cuda, mode):
    """[(A,128)], [(A,128),(B,50)], [(A,70),(B,5)] in one launch, their sequences interleaved: every context's rows are
    bit-identical to its own single-context launch (on the same tensors) and within the fp32 bound"""
    ctxs = [[("A", 128)], [("A", 128), ("B", 50)], [("A", 70), ("B", 5)]]
    own, index = [3, 70, 1, 17, 9, 200, 2], [0, 1, 2, 0, 1, 2, 1]
    H, G = 16, 8
    both = SegProblem(ctxs, own, index, H, G, seed=32)
    out = both.run(cuda, mode)
    check_against_fp32(out, both.reference(mode), int(both.cu_q[-1]), f"three contexts mode={mode}")
    for c, ctx in enumerate(ctxs):
        keep = [s for s, i in enumerate(index) if i == c]
        alone = SegProblem([ctx], [own[s] for s in keep], [0] * len(keep), H, G, seed=77)
        alone.tk, alone.tv = {nm: both.tk[nm] for nm in alone.names}, {nm: both.tv[nm] for nm in alone.names}
        alone.concat()
        for nm in ("q", "k", "v"):
            setattr(alone, nm, torch.cat([getattr(both, nm)[both.cu[s]:both.cu[s + 1]] for s in keep]))
        got = alone.run(cuda, mode)
        for j, s in enumerate(keep):
            assert torch.equal(bits(got[alone.cu[j]:alone.cu[j + 1]]), bits(out[both.cu[s]:both.cu[s + 1]])), \
                f"context {c} sequence {s} changed bits in company"


@pytest.mark.parametrize("mode", [1, 2])
def test_rows_behind_a_use_are_never_read(cuda, mode):
    """[(A,70),(B,5)] on tensors of 128 / 50 rows: NaN in rows >= 70 of A and >= 5 of B changes no bit"""
    p = SegProblem([[("A", 70), ("B", 5)]], OWN, [0, 0, 0], 16, 8, seed=33)
    KV = 2
    p.tk = {"A": rnd(128, KV * D, seed=1), "B": rnd(50, KV * D, seed=2)}
    p.tv = {"A": rnd(128, KV * D, seed=3), "B": rnd(50, KV * D, seed=4)}
    p.concat()
    clean = p.run(cuda, mode)
    nq = int(p.cu_q[-1])
    check_against_fp32(clean, p.reference(mode), nq, f"70+5 mode={mode}")
    tk, tv = {nm: t.clone() for nm, t in p.tk.items()}, {nm: t.clone() for nm, t in p.tv.items()}
    for t in (tk, tv):
        t["A"][70:] = float("nan")
        t["B"][5:] = float("nan")
    dirty = p.run(cuda, mode, tk=tk, tv=tv)
    assert torch.isfinite(dirty[:nq].float()).all()
    assert torch.equal(bits(dirty[:nq]), bits(clean[:nq]))


@pytest.mark.parametrize("mode", [1, 2])
def test_a_plain_launch_gives_the_same_bits_through_both_entries(cuda, mode):
    """no segments: mjv_attention_ctx_bf16 (what ``ops.attention_ctx`` calls for a plain plan) and mjv_attention_ctx_seg_bf16
    with seg == NULL, packed rows and per-context lists"""
    from mj_video_amd import _lib, ops
    p = make_problem([2112, 576], 5, [0, 1, 0, 1, 1], 16, 2, False)
    nq = int(p.cu_q[-1])
    want = p.run(cuda, mode)
    check_against_fp32(want, p.reference(mode), nq, f"plain mode={mode}")
    plan = ops.AttnCtxPlan(p.cu, p.index, p.cu_ctx, p.H, p.G, D, cuda)
    ws = torch.empty(plan.workspace_bytes, dtype=torch.uint8, device=cuda)
    t = {nm: getattr(p, nm).to(cuda) for nm in ("q", "k", "v", "ck", "cv")}
    lib = _lib.load_library()
    lists = torch.tensor([[t["ck"].data_ptr(), t["ck"][2112:].data_ptr()], [t["cv"].data_ptr(), t["cv"][2112:].data_ptr()]],
                         dtype=torch.int64, device=cuda)
    for listed in (False, True):
        out = torch.full((nq + 3, p.H * D), float("nan"), dtype=BF, device=cuda)
        d = plan.desc()
        d.Q, d.K, d.V, d.O = t["q"].data_ptr(), t["k"].data_ptr(), t["v"].data_ptr(), out.data_ptr()
        d.ldq = d.ldo = p.H * D
        d.ldk = d.ldv = d.ld_ctx_k = d.ld_ctx_v = (p.H // p.G) * D
        d.q_head_stride = d.k_head_stride = d.v_head_stride = d.o_head_stride = d.ctx_k_head_stride = d.ctx_v_head_stride = D
        if listed:
            d.ctx_k_list, d.ctx_v_list = lists[0].data_ptr(), lists[1].data_ptr()
        else:
            d.ctx_k, d.ctx_v = t["ck"].data_ptr(), t["cv"].data_ptr()
        d.scale, d.score_round_mode = D ** -0.5, mode
        d.plan, d.plan_ints = plan.plan.data_ptr(), plan.plan_ints
        d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel()
        with torch.cuda.device(cuda):
            rc = lib.mjv_attention_ctx_seg_bf16(C.byref(d), None, torch.cuda.current_stream().cuda_stream)
        assert rc == 0, lib.mjv_last_error()
        torch.cuda.synchronize()
        assert torch.equal(bits(out.cpu()[:nq]), bits(want[:nq])) and torch.isnan(out[nq:].float()).all()


def test_segmented_launch_refusals(cuda):
    """host checks of ``ops.attention_ctx`` and the C entry for a segmented plan, before any launch"""
    from mj_video_amd import _lib, ops
    p = SegProblem([TWO], OWN, [0, 0, 0], 4, 1, seed=34)
    plan = p.plan(cuda)
    ws = torch.empty(plan.workspace_bytes, dtype=torch.uint8, device=cuda)
    out = torch.zeros(int(p.cu_q[-1]), 4 * D, dtype=BF, device=cuda)
    q, k, v = (x.to(cuda) for x in (p.q, p.k, p.v))
    tk, tv = [p.tk[nm].to(cuda) for nm in p.names], [p.tv[nm].to(cuda) for nm in p.names]
    with pytest.raises(ValueError, match="segmented plan needs sequences"):
        ops.attention_ctx(q, k, v, out, p.ck.to(cuda), p.cv.to(cuda), plan, D ** -0.5, 2, ws)
    with pytest.raises(ValueError, match=r"segment tensor 1 \(values\): 36 rows, the longest use of it reads 37"):
        ops.attention_ctx(q, k, v, out, tk, [tv[0], tv[1][:36]], plan, D ** -0.5, 2, ws)
    with pytest.raises(ValueError, match="segments differ"):
        ops.attention_ctx(q, k, v, out, tk, tv, plan, D ** -0.5, 2, ws, segments=[[(0, 100), (1, 36)]])
    with pytest.raises(ValueError, match="segments differ"):
        ops.attention_ctx(q, k, v, out, tk, tv, p.plan(cuda, False), D ** -0.5, 2, ws, segments=p.segments())
    with pytest.raises(_lib.MjvLibraryError, match=r"\(-1\).*workspace"):
        ops.attention_ctx(q, k, v, out, tk, tv, plan, D ** -0.5, 2, ws[:plan.workspace_bytes - 16])
    torch.cuda.synchronize()
    assert not out.float().abs().sum().item(), "a refused call wrote output"
