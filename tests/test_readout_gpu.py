"""mjv_attention_readout_bf16 (include/mjv.h) and model.frame_readout on the MI355X: the kernel against the float64 softmax of the
same bf16 queries / keys (tests/readout_ref.py: reference and bound, worked out from the inputs), untouched memory, equal bits,
independence of the other queries; then the model - layer 0 against the attention probes, bit-identical scores with the readout
on, agreement across prefix_cache / trim_last_layer, frame cutting, score_captions against forward, refusals."""
import contextlib

import numpy as np
import pytest
import torch

from mj_video_amd import layout, ops, synth

import readout_ref
from util import FIELDS, build_hip_model, make_cfg

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
H = 4


# ------------------------------------------------------------------------------------------------ the kernel
def kernel_case(D, G, mode, seed=0):
    """three key tensors that are column ranges of wider rows (one leading dimension), seven queries: key counts 1, 63, 64, 65,
    300 and 4 224; 1, 2 and 3 ranges (a 64-row "prefix" + live rows); two queries on the same tensor with different range_rows"""
    g = torch.Generator().manual_seed(1000 * D + 10 * G + mode + seed)
    KV = H // G
    W = KV * D + 72

    def rnd(rows, cols):
        if mode == 1:   # exactly summable: multiples of 1 / 8 in [-2, 2] - every partial sum of products is exact in fp32
            return (torch.randint(-16, 17, (rows, cols), generator=g).to(torch.float32) / 8).to(BF)
        return torch.randn(rows, cols, generator=g).to(BF)

    wide = [rnd(64, W), rnd(4300, W), rnd(40, W)]
    ranges = [[(1, 5, 1)],
              [(1, 100, 63)],
              [(0, 0, 64)],
              [(0, 0, 64), (1, 7, 1)],
              [(0, 0, 64), (1, 200, 236)],
              [(0, 0, 64), (1, 0, 4120), (2, 0, 40)],
              [(1, 100, 64)]]
    edges = [[0, 1],
             [0, 1, 31, 32, 62, 63],                                        # single keys at the start, in the middle, at the end
             [0, 64],                                                       # one bin
             [0, 64, 65],
             np.round(np.linspace(0, 300, 129)).astype(int).tolist(),       # 128 bins
             [0, 7, 64, 1000, 1001, 2113, 4223, 4224],                      # edges on no chunk boundary (chunks of 264 keys)
             [0, 0, 13, 13, 64]]                                            # empty bins
    q = rnd(len(ranges), H * D + 24)
    return wide, ranges, edges, q


def launch(cuda, wide, ranges, edges, q, D, G, mode, rows=None, ld_mass=130):
    """-> mass [queries + 3, H, ld_mass] (the three extra rows prefilled with NaN, like everything else)"""
    KV = H // G
    sel = list(range(len(ranges))) if rows is None else rows
    plan = ops.AttnReadoutPlan([ranges[i] for i in sel], [edges[i] for i in sel], H, G, D, mode, cuda, n_tensors=len(wide))
    dev_wide = [w.to(cuda) for w in wide]
    tensors = [w[:, 32:32 + KV * D] for w in dev_wide]
    qd = q.to(cuda)[sel][:, 8:8 + H * D]
    mass = torch.full((len(sel) + 3, H, ld_mass), float("nan"), dtype=torch.float32, device=cuda)
    ops.attention_readout(qd, tensors, plan, float(np.float32(D ** -0.5)), mass)
    torch.cuda.synchronize()
    return mass


@pytest.mark.parametrize("mode", [2, 1])
@pytest.mark.parametrize("G", [1, 2])
@pytest.mark.parametrize("D", [128, 96])
def test_kernel_against_float64(cuda, D, G, mode):
    KV = H // G
    wide, ranges, edges, q = kernel_case(D, G, mode)
    mass = launch(cuda, wide, ranges, edges, q, D, G, mode)
    nq = len(ranges)
    host = [w[:, 32:32 + KV * D] for w in wide]
    ref, bound, sum_bound = readout_ref.reference(q[:, 8:8 + H * D].reshape(nq, H, D), host, ranges, edges, G, D, D ** -0.5, mode, ld_mass=130)
    got = mass[:nq].cpu()
    readout_ref.check(got, ref, bound, f"D {D} G {G} mode {mode}")
    # every (query, head) sums to 1
    sums = got.to(torch.float64).sum(dim=2)
    print("max |sum - 1| =", (sums - 1).abs().max().item(), "bound", sum_bound.min().item(), "..", sum_bound.max().item())
    assert ((sums - 1).abs() <= sum_bound).all()
    # untouched memory: the extra rows stay NaN, bins beyond a query's count are exactly 0
    assert torch.isnan(mass[nq:]).all()
    for i, e in enumerate(edges):
        assert (got[i, :, len(e) - 1:] == 0).all(), i
        assert not torch.isnan(got[i]).any()
    assert (got[6, :, 0] == 0).all() and (got[6, :, 2] == 0).all()      # empty bins
    # two launches give equal bits
    again = launch(cuda, wide, ranges, edges, q, D, G, mode)
    assert torch.equal(mass[:nq].view(torch.int32), again[:nq].view(torch.int32))
    # a query's bits do not change when other queries join the launch (or when it moves within it)
    for rows in ([4], [5, 1], [6, 3, 0]):
        alone = launch(cuda, wide, ranges, edges, q, D, G, mode, rows=rows)
        for j, i in enumerate(rows):
            assert torch.equal(alone[j].view(torch.int32), mass[i].view(torch.int32)), (rows, i)


def test_kernel_five_key_counts_in_one_launch_and_strides(cuda):
    """five queries of different key counts over ONE tensor, a q_head_stride and k_head_stride wider than the head"""
    D, G, mode = 128, 2, 2
    KV = H // G
    g = torch.Generator().manual_seed(5)
    khs, qhs = D + 16, D + 8
    k = torch.randn(700, KV * khs, generator=g).to(BF)
    q = torch.randn(5, H * qhs, generator=g).to(BF)
    lens = [1, 17, 129, 333, 700]
    ranges = [[(0, 0, n)] for n in lens]
    edges = [[0, n] if n < 3 else [0, 1, n - 1, n] for n in lens]
    plan = ops.AttnReadoutPlan(ranges, edges, H, G, D, mode, cuda)
    mass = torch.full((5, H, 3), float("nan"), dtype=torch.float32, device=cuda)
    ops.attention_readout(q.to(cuda), [k.to(cuda)], plan, D ** -0.5, mass, q_head_stride=qhs, k_head_stride=khs)
    torch.cuda.synchronize()
    qh = torch.stack([q[:, h * qhs:h * qhs + D] for h in range(H)], dim=1)
    ref, bound, _ = readout_ref.reference(qh, [k], ranges, edges, G, D, D ** -0.5, mode, khs=khs, ld_mass=3)
    readout_ref.check(mass.cpu(), ref, bound, "five key counts")


def test_kernel_launch_refusals(cuda):
    D, G = 128, 2
    k = torch.zeros(64, (H // G) * D, dtype=BF, device=cuda)
    q = torch.zeros(1, H * D, dtype=BF, device=cuda)
    plan = ops.AttnReadoutPlan([[(0, 0, 64)]], [[0, 10, 64]], H, G, D, 2, cuda)
    ops.prof_enable(True)
    ops.prof_reset()
    try:
        with pytest.raises(ValueError, match="row 64"):    # a range past its tensor's rows never reaches the kernel
            ops.attention_readout(q, [k[:63]], plan, 1.0, torch.zeros(1, H, 2, device=cuda))
        with pytest.raises(ValueError, match="mass"):
            ops.attention_readout(q, [k], plan, 1.0, torch.zeros(1, H, 1, device=cuda))
        with pytest.raises(ValueError, match="2 key tensors"):
            ops.attention_readout(q, [k, k], plan, 1.0, torch.zeros(1, H, 2, device=cuda))
        assert not ops.prof_results(), "a refused call launched something"
    finally:
        ops.prof_enable(False)
        ops.prof_reset()


# ------------------------------------------------------------------------------------------------ the model
def tiny_model(cuda, tower):
    """tiny InternLM2 (head_dim 128, 2 q-heads per kv head) / tiny Phi-3 (head_dim 96, MHA) at 56^2, no GEMM slicing K"""
    import copy
    from mj_video_amd import configuration as C
    from mj_video_amd.modeling import InternVLChatRewardModeling
    if tower == "internlm2":
        cfg, tk = make_cfg("tiny", 56), synth.INTERNLM2_TOKENS
        model = build_hip_model(cfg, synth.synth_state_dict(cfg, seed=0), cuda)
    else:
        cfg = C.InternVLChatRewardModelingConfig(**copy.deepcopy(C.tiny_phi3_config_dict(56)), **C.mjvideo_head_kwargs())
        tk = synth.PHI3_TOKENS
        model = InternVLChatRewardModeling.from_config(cfg, dtype=BF)
        model.load_state_dict(synth.synth_state_dict(cfg, seed=3), strict=True)
        model.config.pad_token_id = tk.pad
        model = model.to(BF).to(cuda).eval()
        model.model.img_context_token_id = tk.img_context
    model.use_gemm_workspace = False
    model.attention_scores = "flash"
    return model, cfg, tk


def batch_of(cfg, tk, videos, cuda):
    from mj_video_amd.chat_input import num_image_tokens_per_tile
    per = num_image_tokens_per_tile(cfg)
    px = [synth.synth_pixel_values(300, i, t, 56) for i, (t, _) in enumerate(videos)]
    ids = [synth.synth_input_ids(per * t, 10 + i, interleave_frames=inter, tokens=tk) for i, (t, inter) in enumerate(videos)]
    ids_b, mask = synth.pad_batch(ids, pad_id=tk.pad)
    return torch.cat(px).to(cuda), ids_b.to(cuda), mask.to(cuda)


MIXED = [(4, 4), (2, None), (3, 3)]      # (tiles, interleaved frame labels): tile counts 4, 2, 3


@contextlib.contextmanager
def recorded():
    """every launch of the readout with copies of its queries and key tensors"""
    calls, real = [], ops.attention_readout

    def spy(q, k_tensors, plan, scale, mass, **kw):
        calls.append(dict(q=q[:plan.n_queries].clone(), tensors=[t.clone() for t in k_tensors], plan=plan, scale=scale))
        return real(q, k_tensors, plan, scale, mass, **kw)

    ops.attention_readout = spy
    try:
        yield calls
    finally:
        ops.attention_readout = real


def fold_public(bin_mass, bins, F_max):
    """[2 B, H, bins] (reward rows, then gating rows) -> [B, 2, H, F_max + 2] by the fold maps of layout.readout_bins"""
    B = len(bins)
    out = torch.zeros(B, 2, bin_mass.shape[1], F_max + 2, dtype=torch.float64)
    for b, sample in enumerate(bins):
        for i, row in enumerate((sample.reward, sample.gating)):
            for j, col in enumerate(row.fold.tolist()):
                out[b, i, :, col if col < sample.n_frames else col - sample.n_frames + F_max] += bin_mass[i * B + b, :, j]
    return out


def reference_of_calls(calls, bins, model):
    """the float64 reference and the bound of every recorded launch, folded: ([B, 2, layers, H, F_max + 2], [B, 2, layers, H, 1])"""
    Hh, KV, G, hd, scale, mode = model._llm_geom()
    F_max, B = max(s.n_frames for s in bins), len(bins)
    refs, bounds = [], []
    for c in calls:
        p = c["plan"]
        ranges = [[(int(p.range_tensor[r]), int(p.range_row0[r]), int(p.range_rows[r])) for r in range(p.cu_range[i], p.cu_range[i + 1])]
                  for i in range(p.n_queries)]
        edges = [p.bin_edge[p.cu_bin[i]:p.cu_bin[i + 1]].tolist() for i in range(p.n_queries)]
        ref, bound, _ = readout_ref.reference(c["q"].cpu().view(p.n_queries, Hh, hd), [t.cpu() for t in c["tensors"]], ranges, edges, G, hd,
                                              c["scale"], mode)
        refs.append(fold_public(ref, bins, F_max))
        bounds.append(bound.view(2, B, Hh, 1).transpose(0, 1))
    return torch.stack(refs, dim=2), torch.stack(bounds, dim=2)


def host_bins(model, ids, mask, tiles_per_frame=1):
    rules = model._token_rules()
    ids, mask = ids.cpu().numpy(), mask.cpu().numpy().astype(bool)
    return [layout.readout_bins(rules, ids[b], np.flatnonzero(mask[b]), tiles_per_frame) for b in range(ids.shape[0])]


_RUNS = {}


def forward_runs(cuda, tower):
    """the MIXED batch under every (prefix_cache, trim_last_layer) setting with the readout on, and the float64 reference of the
    launches of the plain setting - computed once per tower, shared by the tests below"""
    if tower in _RUNS:
        return _RUNS[tower]
    model, cfg, tk = tiny_model(cuda, tower)
    px, ids, mask = batch_of(cfg, tk, MIXED, cuda)
    model.frame_readout = True
    runs = {}
    for cache, trim in ((False, False), (True, True), (True, False), (False, True), (True, True)):
        model.prefix_cache, model.trim_last_layer = cache, trim
        with recorded() as calls:
            out = model.forward(px, ids, mask)
        torch.cuda.synchronize()
        runs[(cache, trim)] = dict(out=out, mass=model.last_readout.mass.clone(), n_frames=model.last_readout.n_frames, calls=calls,
                                   readout=model.last_readout)
    bins = host_bins(model, ids, mask)
    ref, bound = reference_of_calls(runs[(False, False)]["calls"], bins, model)
    _RUNS[tower] = dict(model=model, cfg=cfg, tk=tk, px=px, ids=ids, mask=mask, runs=runs, bins=bins, ref=ref, bound=bound)
    return _RUNS[tower]


@pytest.mark.parametrize("tower", ["internlm2", "phi3"])
def test_model_layer0_against_the_probes(cuda, tower):
    """(a) the layer-0 mass of both rows of every sample = the float64 softmax of the attention probe's rows (llm_attn0: the q / k
    the first causal attention read), binned by layout.readout_bins; the kernel's bound"""
    R = forward_runs(cuda, tower)
    model, px, ids, mask, bins = R["model"], R["px"], R["ids"], R["mask"], R["bins"]
    Hh, KV, G, hd, scale, mode = model._llm_geom()
    model.frame_readout, model.debug_probes = False, {}
    try:
        model.forward(px, ids, mask)
        torch.cuda.synchronize()
        probe = model.debug_probes["llm_attn0"]
    finally:
        model.debug_probes, model.frame_readout = None, True
    q, k = probe["q"].cpu(), probe["k"].cpu()
    B = ids.shape[0]
    cu = np.concatenate([[0], np.cumsum(mask.cpu().numpy().sum(axis=1))])
    rows = [s.reward for s in bins] + [s.gating for s in bins]
    ranges = [[(0, int(cu[i % B]), row.keys)] for i, row in enumerate(rows)]
    qs = torch.stack([q[int(cu[i % B]) + row.keys - 1] for i, row in enumerate(rows)]).view(2 * B, Hh, hd)
    ref, bound, _ = readout_ref.reference(qs, [k], ranges, [row.edges.tolist() for row in rows], G, hd, scale, mode)
    F_max = max(s.n_frames for s in bins)
    ref, bound = fold_public(ref, bins, F_max), bound.view(2, B, Hh, 1).transpose(0, 1)
    assert R["runs"][(True, True)]["n_frames"].tolist() == [4, 2, 3] and F_max == 4
    for key, run in R["runs"].items():
        mass = run["mass"]
        assert mass.shape == (B, 2, len(model.model.language_model.model.layers), Hh, F_max + 2) and mass.dtype == torch.float32
        readout_ref.check(mass[:, :, 0].cpu(), ref, bound, f"{tower} layer 0 vs probes, prefix_cache / trim {key}")
        # frames a sample does not have are exactly 0; every row's columns sum to 1
        assert (mass[1, :, :, :, 2:4] == 0).all() and (mass[2, :, :, :, 3] == 0).all()
        assert ((mass.double().sum(dim=-1) - 1).abs() < 1e-5).all()
    # per_frame: the mean over heads and layers
    ro = R["runs"][(True, True)]["readout"]
    assert torch.equal(ro.per_frame(), ro.mass[:, 0, :, :, :F_max].mean(dim=(1, 2))) and ro.per_frame("gating", layers=[0]).shape == (B, F_max)


@pytest.mark.parametrize("tower", ["internlm2", "phi3"])
def test_model_scores_keep_their_bits_and_launches(cuda, tower):
    """(b) every CustomOutput field is bit-identical with the readout on and off; off, a forward launches no readout kernel and
    leaves last_readout None; on, it adds one readout launch and one row gather per decoder layer and nothing else"""
    R = forward_runs(cuda, tower)
    model, px, ids, mask = R["model"], R["px"], R["ids"], R["mask"]
    layers = len(model.model.language_model.model.layers)
    tags = {}
    ops.prof_enable(True)
    try:
        for on in (False, True):
            model.frame_readout, model.prefix_cache, model.trim_last_layer = on, True, True
            ops.prof_reset()
            out = model.forward(px, ids, mask)
            tags[on] = {t: r["launches"] for t, r in ops.prof_results().items()}
            if on:
                assert model.last_readout is not None
                for f in FIELDS:
                    assert torch.equal(getattr(out, f), getattr(off_out, f)), f
                    assert torch.equal(getattr(out, f), getattr(R["runs"][(True, True)]["out"], f)), f
            else:
                assert model.last_readout is None
                off_out = out
    finally:
        ops.prof_enable(False)
        ops.prof_reset()
        model.frame_readout = True
    tag = f"attn_readout_d{model._llm_geom()[3]}"
    assert not [t for t in tags[False] if t.startswith("attn_readout")], tags[False]
    expect = dict(tags[False])
    expect[tag] = layers
    expect["embed_gather"] = expect.get("embed_gather", 0) + layers
    assert tags[True] == expect, (tags[True], expect)


@pytest.mark.parametrize("tower", ["internlm2", "phi3"])
def test_model_switches(cuda, tower):
    """(c) the masses with prefix_cache / trim_last_layer on agree with those with both off within twice the kernel's bound (the
    ranges are cut differently: only the summation order may differ), and each setting's own launches hold the kernel's bound
    against the float64 reference of the plain setting's queries and keys - in EVERY layer"""
    R = forward_runs(cuda, tower)
    ref, bound, runs = R["ref"], R["bound"], R["runs"]
    plain = runs[(False, False)]["mass"].cpu()
    readout_ref.check(plain, ref, bound, f"{tower} plain setting, all layers")
    for key in ((True, True), (True, False), (False, True)):
        got = runs[key]["mass"].cpu()
        diff = (got.double() - plain.double())
        print(f"{tower} {key}: rms of the difference to the plain setting = {diff.pow(2).mean().sqrt().item():.3e}")
        readout_ref.check(got, plain.double(), bound, f"{tower} prefix_cache / trim {key} vs both off", factor=2.0)
    assert len(runs[(True, True)]["calls"][0]["tensors"]) == 2 and len(runs[(False, False)]["calls"][0]["tensors"]) == 1


@pytest.mark.parametrize("tower", ["internlm2", "phi3"])
def test_model_frame_cutting(cuda, tower):
    """(d) tiles_per_frame [2, 1, 1] on four-tile videos (frame labels between the tiles / one long run): the columns of
    tiles_per_frame 1 with the first two frames summed - exact up to fp32 addition"""
    R = forward_runs(cuda, tower)
    model, cfg, tk = R["model"], R["cfg"], R["tk"]
    px, ids, mask = batch_of(cfg, tk, [(4, 4), (4, None)], cuda)
    model.prefix_cache = model.trim_last_layer = True
    try:
        model.readout_tiles_per_frame = 1
        model.forward(px, ids, mask)
        one = model.last_readout.mass.double().cpu()
        model.readout_tiles_per_frame = [2, 1, 1]
        model.forward(px, ids, mask)
        cut = model.last_readout
    finally:
        model.readout_tiles_per_frame = 1
    assert cut.n_frames.tolist() == [3, 3] and cut.mass.shape[-1] == 5 and one.shape[-1] == 6
    want = torch.cat([one[..., 0:1] + one[..., 1:2], one[..., 2:]], dim=-1)
    d = (cut.mass.double().cpu() - want).abs().max().item()
    print(f"{tower}: frame cutting, max difference {d:.3e}")
    assert d <= 1e-6


def test_model_score_captions_against_forward(cuda):
    """(e) InternLM2: score_captions over one plain context and one extend_context child against forward on the same full
    prompts, per row and layer: twice the kernel's bound plus the allowance for differing hidden states, taken as 2 x the rms
    that forward's masses show between prefix_cache on and off in (c)"""
    from mj_video_amd import harness
    from mj_video_amd.chat_input import num_image_tokens_per_tile
    R = forward_runs(cuda, "internlm2")
    model, cfg, tk = R["model"], R["cfg"], R["tk"]
    rms_c = (R["runs"][(True, False)]["mass"].double() - R["runs"][(False, False)]["mass"].double()).pow(2).mean().sqrt().item()
    per = num_image_tokens_per_tile(cfg)
    px = synth.synth_pixel_values(300, 5, 4, 56).to(cuda)
    prompts = [synth.synth_input_ids(4 * per, 40 + i, n_caption=n) for i, n in enumerate((4, 9, 24))]
    ids, mask = synth.pad_batch(prompts)
    ids, mask = ids.to(cuda), mask.to(cuda)
    model.prefix_cache = model.trim_last_layer = True
    with recorded() as calls:
        model.forward(torch.cat([px] * 3), ids, mask)
    torch.cuda.synchronize()
    fwd = model.last_readout.mass.cpu()
    bins = host_bins(model, ids, mask)
    ref, bound = reference_of_calls(calls, bins, model)
    readout_ref.check(fwd, ref, bound, "forward on the caption prompts")
    parent = model.encode_video(px, prompts[0])
    K = harness.shared_prefix_len(prompts, synth.PAD_ID)
    child = model.extend_context(parent, prompts[0], context_len=K)
    assert len(child.segments) == 2
    out = model.score_captions([parent, child], ids, mask, context_index=[0, 1, 0])
    torch.cuda.synchronize()
    cap = model.last_readout
    assert cap.mass.shape == fwd.shape and cap.n_frames.tolist() == [4, 4, 4]
    diff = cap.mass.double().cpu() - fwd.double()
    print(f"score_captions vs forward: rms of the difference {diff.pow(2).mean().sqrt().item():.3e}, max {diff.abs().max().item():.3e}; "
          f"allowance 2 x rms of (c) = {2 * rms_c:.3e}")
    readout_ref.check(cap.mass.cpu(), fwd.double(), bound, "score_captions vs forward", factor=2.0, extra=2 * rms_c)
    model.frame_readout = False
    try:
        off = model.score_captions([parent, child], ids, mask, context_index=[0, 1, 0])
        assert model.last_readout is None
        for f in FIELDS:
            assert torch.equal(getattr(out, f), getattr(off, f)), f
    finally:
        model.frame_readout = True


@pytest.mark.parametrize("tower", ["internlm2", "phi3"])
def test_model_refusals(cuda, tower):
    """(f) norm_fusion with the readout on: NotImplementedError; a tiles_per_frame that does not account for the image tokens:
    ValueError before anything is launched"""
    R = forward_runs(cuda, tower)
    model, px, ids, mask = R["model"], R["px"], R["ids"], R["mask"]
    ops.prof_enable(True)
    ops.prof_reset()
    try:
        model.readout_tiles_per_frame = [2, 1, 1]          # fits the first sample (4 tiles), not the second (2)
        with pytest.raises(ValueError, match="tiles_per_frame"):
            model.forward(px, ids, mask)
        model.readout_tiles_per_frame = 1
        model.norm_fusion = True
        with pytest.raises(NotImplementedError, match="norm_fusion"):
            model.forward(px, ids, mask)
        assert not ops.prof_results(), "a refused call launched something"
    finally:
        model.norm_fusion, model.readout_tiles_per_frame = False, 1
        ops.prof_enable(False)
        ops.prof_reset()
    assert model.last_readout is None


def test_harness_score_with_frame_readout(cuda):
    """harness.score_with_frame_readout: the scores of a plain forward on the same prompt, bit for bit, and the readout of its
    frames; tiles_per_frame 2 sums pairs of frames; the model's switches are restored"""
    from mj_video_amd import harness
    from mj_video_amd.chat_input import prepare_chat_input, video_prefix
    from test_host_logic import StubTokenizer
    R = forward_runs(cuda, "internlm2")
    model, cfg = R["model"], R["cfg"]
    tok, caption = StubTokenizer(), "a cat walks over a red carpet"
    pv = synth.synth_pixel_values(31, 2, 4, 56).to(cuda)
    model.frame_readout = False
    try:
        out, ro = harness.score_with_frame_readout(model, cfg, tok, pv, caption, {})
        assert model.frame_readout is False and model.readout_tiles_per_frame == 1
        ids, mask = prepare_chat_input(cfg, tok, pv, video_prefix(4) + caption, {}, device="cpu")
        plain = model.forward(pv, ids.to(cuda), mask.to(cuda))
        assert model.last_readout is None
        for f in FIELDS:
            assert torch.equal(getattr(out, f), getattr(plain, f)), f
        Hh, layers = model._llm_geom()[0], len(model.model.language_model.model.layers)
        assert ro.mass.shape == (1, 2, layers, Hh, 6) and ro.n_frames.tolist() == [4] and ro.per_frame().shape == (1, 4)
        assert ((ro.mass.double().sum(dim=-1) - 1).abs() < 1e-5).all() and (ro.mass[..., :4] > 0).all()
        _, two = harness.score_with_frame_readout(model, cfg, tok, pv, caption, {}, tiles_per_frame=2)
        one = ro.mass.double()
        want = torch.stack([one[..., 0] + one[..., 1], one[..., 2] + one[..., 3], one[..., 4], one[..., 5]], dim=-1)
        assert two.n_frames.tolist() == [2] and (two.mass.double() - want).abs().max().item() <= 1e-6
    finally:
        model.frame_readout = True
