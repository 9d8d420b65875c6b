"""The reference helpers of tests/rowops_ref.py against torch's own bf16 modules, on the CPU (no GPU needed), and the
caps test_rowops_gpu.py holds the kernels to, shown to hold for a reference-grade fp32 implementation alone.

RoPE must be bit-identical to the elementwise bf16 formula; the norms within 1 bf16 ulp of torch's bf16 LayerNorm / the InternLM2
RMSNorm formula (the bit-identical share is printed; measured: LayerNorm 0.99997 - 1.0, RMSNorm 0.9999 - 1.0).  The one-hot
and uniform reward-heads cases must be exact: every fp32 sum of their matvecs is exactly representable, and the fp64 restatement
agrees with the torch bf16 restatement bit for bit.
"""
import pytest
import torch
import torch.nn.functional as F

import rowops_ref as R

BF = torch.bfloat16


def test_round_bf16_has_no_double_rounding():
    v = torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -30, 1.0 + 2.0 ** -8 - 2.0 ** -30, -(1.0 + 2.0 ** -8 + 2.0 ** -30), 1.0 + 2.0 ** -8,
                      1.0 + 3 * 2.0 ** -8, 0.0, 3e4], dtype=torch.float64)
    got = R.round_bf16(v).double()
    want = torch.tensor([1.0 + 2.0 ** -7, 1.0, -(1.0 + 2.0 ** -7), 1.0, 1.0 + 2.0 ** -6, 0.0, 29952.0], dtype=torch.float64)
    assert torch.equal(got, want), (got, want)
    x = torch.randn(4096, generator=R.gen(1), dtype=torch.float64)
    assert torch.equal(R.round_bf16(x.float().double()), x.float().to(BF))       # fp32-representable values: torch's own rounding


def test_ulps_is_the_suite_s_bf16_ulps():
    from util import bf16_ulps
    a, b = R.randn_bf16(R.gen(2), 5000), R.randn_bf16(R.gen(3), 5000)
    assert torch.equal(R.ulps(a, b), bf16_ulps(a, b))
    one = torch.tensor([1.0, -1.0, 0.0], dtype=BF)
    nxt = torch.tensor([1.0078125, -1.0078125, 9.1835e-41], dtype=BF)
    assert R.ulps(one, nxt).tolist() == [1, 1, 1]
    assert torch.equal(R.bf16_ulp(torch.tensor([1.0, 1.9, 2.0, 0.3])), torch.tensor([2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -9],
                                                                                        dtype=torch.float64))


@pytest.mark.parametrize("D,base,factor", [(128, 1e6, 1.0), (96, 1e4, 1.19), (48, 1e4, 1.19), (32, 1e4, 1.0), (64, 1e4, 1.0)])
def test_rope_ref_is_bit_identical_to_the_bf16_formula(D, base, factor):
    cos, sin = R.rope_tables(300, D, base, factor)
    x = R.randn_bf16(R.gen(D), 300, 5, D, std=2.0)
    pos = torch.randint(0, 300, (300,), generator=R.gen(D + 1))
    c, s = cos[pos][:, None, :], sin[pos][:, None, :]
    assert torch.equal(R.rope_ref(x, c, s), R.rope_torch(x, c, s))


@pytest.mark.parametrize("dim", [8, 520, 1024, 3080, 4096])
def test_norm_refs_against_torch_bf16_modules(dim):
    x = R.randn_bf16(R.gen(dim), 257, dim)
    g, b = R.gain_bias(dim, dim + 1)
    ref, floor, _, _ = R.layernorm_ref(x, g, b, 1e-6)
    tor = F.layer_norm(x, (dim,), g, b, 1e-6)                       # nn.LayerNorm on a bf16 tensor
    u = R.ulps(ref, tor)
    print(f"layernorm_ref vs F.layer_norm(bf16), dim {dim}: max {int(u.max())} ulps, bit-identical share {(u == 0).float().mean():.4f}")
    # 1 ulp - or the cancellation floor: at dim 3080 one element is 5.3e-7 where beta = 0.176 (x_hat * gamma cancels beta to
    # 3e-6 of its size), and there torch's fp32 arithmetic is 3 ulps of that remainder (1.1e-8) away, under the floor of 3.9e-6
    R.assert_norm(R.norm_report(tor, ref, floor), "layernorm_ref vs torch bf16")
    ref, _, _, _ = R.rmsnorm_ref(x, g, 1e-5)
    h = x.to(torch.float32)                                         # InternLM2RMSNorm.forward, line by line
    h = h * torch.rsqrt(h.pow(2).mean(-1, keepdim=True) + 1e-5)
    tor = g * h.to(BF)
    u = R.ulps(ref, tor)
    print(f"rmsnorm_ref vs InternLM2RMSNorm formula, dim {dim}: max {int(u.max())} ulps, bit-identical share {(u == 0).float().mean():.4f}")
    assert int(u.max()) <= 1


@pytest.mark.parametrize("regime", R.REGIMES)
@pytest.mark.parametrize("dim", R.REGIME_WIDTHS)
def test_norm_caps_hold_for_an_fp32_implementation(regime, dim):
    """The rule of test_rowops_gpu.py (1 ulp of the rounded fp64 reference, or the 2^-20 cancellation floor; the floor alone on
    constant and zero rows; N(0,1): 0.98 bit-identical) applied to torch's fp32 LayerNorm / the fp32 RMSNorm formula: a
    reference-grade implementation passes it in every regime, so the rule asks nothing a correct kernel cannot give.  RMSNorm
    needs the alternatives of rmsnorm_ref for that: without them the fp32 formula itself is 2 ulps off on 6 of 4.2 M elements.
    Measured shares (fp32 torch vs the fp64 reference, smallest over the widths), LayerNorm / RMSNorm: normal 0.99998 / 0.99999,
    mean64 0.9966 / 1.0, massive 0.9999 / 1.0, tiny 0.9999 / 1.0, alternating 0.9955 / 1.0 (constant and zero rows: bit-identical)."""
    rows = 1025 if regime in ("normal", "massive") else 65
    x = R.regime_rows(regime, rows, dim, seed=dim + 7)
    g, b = R.gain_bias(dim, dim + 1)
    flat = regime in ("constant", "zero")
    ref, floor, _, _ = R.layernorm_ref(x, g, b, 1e-6)
    rep = R.norm_report(R.layernorm_f32(x, g, b, 1e-6), ref, floor, floor_only=flat)
    print(f"fp32 LayerNorm, {regime} x {dim}: {rep}")
    R.assert_norm(rep, f"fp32 layernorm {regime}", 0.98 if regime == "normal" else None)
    ref, floor, _, alts = R.rmsnorm_ref(x, g, 1e-5)
    rep = R.norm_report(R.rmsnorm_f32(x, g, 1e-5), ref, floor, floor_only=flat, alts=alts)
    print(f"fp32 RMSNorm, {regime} x {dim}: {rep}")
    R.assert_norm(rep, f"fp32 rmsnorm {regime}", 0.98 if regime == "normal" else None)


@pytest.mark.parametrize("dim", R.REGIME_WIDTHS)
def test_row_stats_caps_hold_for_an_fp32_two_pass(dim):
    """the N(0,1) tolerances of test_row_stats (rstd rtol 2e-6; mean * rstd rtol 2e-5 / atol 1e-6) hold for an fp32 two-pass
    computation on the CPU, and in every other regime its error - the yardstick the kernel gets 4 x of - is finite"""
    for regime in R.REGIMES:
        x = R.regime_rows(regime, 65, dim, seed=dim + 9)
        for mean in (True, False):
            eps = 1e-6 if mean else 1e-5
            r32, m32 = R.row_stats_f32(x, eps, mean)
            r64, m64 = R.row_stats_ref(x, eps, mean)
            rel = ((r32.double() - r64).abs() / r64).max().item()
            print(f"fp32 two-pass rstd, {regime} x {dim}, mean={mean}: max rel err {rel:.3e}")
            assert rel < 1e-5
            if regime == "normal":
                assert torch.allclose(r32.double(), r64, rtol=2e-6, atol=0)
                if mean:
                    assert torch.allclose(m32.double(), m64, rtol=2e-5, atol=1e-6)


def test_pixel_shuffle_rows_is_the_reference_s_view_permute_chain():
    tiles, G, d = 2, 6, 16
    x = R.randn_bf16(R.gen(5), tiles * (G * G + 1), d)
    v = x.view(tiles, G * G + 1, d)[:, 1:, :].reshape(tiles, G, G, d)      # modeling_internvl_chat.py: pixel_shuffle, ps_version v2
    n, w_, h_, c = v.shape
    v = v.view(n, w_, h_ // 2, c * 2).permute(0, 2, 1, 3).contiguous()
    v = v.view(n, h_ // 2, w_ // 2, c * 4).permute(0, 2, 1, 3).contiguous().view(-1, 4 * d)
    assert torch.equal(R.pixel_shuffle_rows(x, tiles, G), v)


HEADS_SHAPES = [(5, 1, 1, [[0]], 8, 8), (5, 5, 5, [[3], [0], [4], [1], [2]], 520, 1032), (7, 28, 5, R.product_groups(), 2048, 1024),
                (7, 64, 16, R.strided_groups(64, 16, 5), 3072, 1032), (7, 64, 1, R.strided_groups(64, 1, 7), 520, 8)]


@pytest.mark.parametrize("regime", ["onehot", "uniform"])
@pytest.mark.parametrize("T", [1.0, 0.5, 4.0])
@pytest.mark.parametrize("B,n_obj,n_asp,groups,hidden,gate_hidden", HEADS_SHAPES)
def test_exact_heads_cases_are_exact(regime, T, B, n_obj, n_asp, groups, hidden, gate_hidden):
    """one-hot and uniform cases: every matvec sum is exactly representable in fp32 (so its value does not depend on the
    summation order and its bf16 rounding is the same everywhere), no rounding is ambiguous, and the fp64 restatement equals the
    torch bf16 restatement bit for bit; one-hot weights are exactly 0 or logit_scale"""
    p = R.heads_case(31, B, n_obj, n_asp, groups, hidden, gate_hidden, T, regime)
    for a, w, bias in ((p["hr"], p["w_reg"], None), (p["ga"], p["wa"], p["ba"]), (p["gc"], p["wc"], p["bc"])):
        v, mag, _, _ = R._matvec(a, w, bias)
        quantum = 2.0 ** -6
        assert torch.equal(v, torch.round(v / quantum) * quantum) and float(mag.max()) < 2.0 ** 24 * quantum   # integers * 2^-6 below 2^24
    o = R.heads_ref(p)
    v1 = R.rb(p["hr"].double() @ p["w_reg"].double().t()) @ p["w_transform"].double()
    assert torch.equal(v1, v1.float().double()) and float(o["rewards_mag"].max()) < 2.0 ** 24 * 2.0 ** -16
    t = R.heads_torch(p)
    for f in ("rewards", "criteria_gating", "aspect_gating", "aspect_weights", "weighted_last"):
        assert torch.equal(R.round_bf16(o[f]), t[f]), f
    assert torch.equal(o["aspect_scores"].float(), t["aspect_scores"])
    if regime == "onehot":
        w, ag = o["aspect_weights"], o["aspect_gating"]
        assert (((w == 0) | (w == 0.75)).all() and (w == 0.75).sum() == B * n_asp), "one-hot criteria weights"
        assert (((ag == 0) | (ag == 1.5)).all() and (ag == 1.5).sum() == B), "one-hot aspect gating"
        assert torch.equal(o["score"].float(), t["score"])
    else:
        sizes = torch.tensor([len(g) for g in groups for _ in g], dtype=torch.float64)
        assert torch.equal(o["aspect_weights"], R.rb(R.rb(1.0 / sizes) * 0.75).expand(B, -1))
        assert ((o["score"] - t["score"].double()).abs() <= 1e-6 * o["score_mag"]).all()


@pytest.mark.parametrize("B,n_obj,n_asp,groups,hidden,gate_hidden", HEADS_SHAPES)
def test_heads_restatements_agree_on_random_inputs(B, n_obj, n_asp, groups, hidden, gate_hidden):
    """N(0,1) inputs: the torch bf16 restatement against the fp64 one within the end-to-end bounds of
    test_reward_heads_kernel_against_oracle (2 ulps or 1e-3; fp32 fields 1 % + 2e-3) - two independent restatements of one
    piece of arithmetic"""
    p = R.heads_case(32, 40, n_obj, n_asp, groups, hidden, gate_hidden, 1.0, "normal")
    o, t = R.heads_ref(p), R.heads_torch(p)
    for f in ("rewards", "criteria_gating", "aspect_gating", "aspect_weights", "weighted_last"):
        got, exp = t[f].double(), o[f]
        ok = (R.ulps(t[f], R.round_bf16(exp)) <= 2) | ((got - exp).abs() <= 1e-3)
        assert ok.all(), f
    for f in ("aspect_scores", "score"):
        assert ((t[f].double() - o[f]).abs() <= 0.01 * o[f].abs() + 2e-3).all(), f
