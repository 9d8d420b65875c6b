"""Plain fp64 references of the row kernels (rowops.hip) and the reward heads (heads.hip), with the bf16 rounding points
include/mjv.h states, plus the seeded input generators and the comparison rules of test_rowops_refs.py (CPU) and
test_rowops_gpu.py (MI355X).  Test infrastructure only; imports nothing but torch, so the CPU tests need no GPU.

How the bounds are derived (every figure is used by name below):
  * a bf16 value has 8 significant bits: one unit in the last place is 2^-8 .. 2^-7 of the value;
  * an fp32 sum of n terms, summed in any order, is off by at most about n * 2^-24 of the summed magnitudes, and by far less
    on average.  2^-20 of the summed (cancelling) magnitude is the allowance test_gemm_folded_layernorm already grants; here
    it is FLOOR_REL.  A kernel and a reference that agree to that accuracy before a bf16 rounding can land on different sides
    of a rounding boundary: one ulp after one rounding point, two after two.
"""
import math

import torch
import torch.nn.functional as F

BF = torch.bfloat16
F64 = torch.float64
FLOOR_REL = 2.0 ** -20
FP32_HALF_ULP = 2.0 ** -24

NORM_WIDTHS = (8, 128, 520, 1024, 1032, 1536, 2048, 2056, 3072, 3080, 4096)
NORM_ROWS = (1, 3, 4, 5, 1025)
REGIME_WIDTHS = (1024, 2048, 3072, 4096)
REGIMES = ("normal", "mean64", "constant", "zero", "massive", "tiny", "alternating")
SENTINEL = -1234.0       # bf16-exact; what padding columns and never-written rows hold before a launch


# ------------------------------------------------------------------------------------------------ rounding
def round_bf16(t: torch.Tensor) -> torch.Tensor:
    """fp64 (or fp32) -> the NEAREST bf16, ties to even.  torch converts fp64 -> fp32 -> bf16; the first rounding can land
    exactly on a bf16 tie the fp64 value was not on (1 + 2^-8 + 2^-30 becomes the tie 1 + 2^-8 and then rounds to even,
    down).  Such a value is moved one fp32 step back towards the fp64 value before the second rounding."""
    if t.dtype != F64:
        return t.to(BF)
    f = t.to(torch.float32)
    bits = f.view(torch.int32)
    d = t - f.double()
    tie = ((bits & 0xFFFF) == 0x8000) & (d != 0) & torch.isfinite(f)
    step = torch.where((d > 0) == (f > 0), 1, -1).to(torch.int32)      # +1 = away from zero in the sign-magnitude pattern
    return torch.where(tie, bits + step, bits).view(torch.float32).to(BF)


def rb(t: torch.Tensor) -> torch.Tensor:
    """one bf16 rounding point inside an fp64 computation"""
    return round_bf16(t).to(F64)


def bf16_ulp(t: torch.Tensor) -> torch.Tensor:
    """size of one bf16 unit in the last place at the magnitude of ``t`` (fp64 out)"""
    a = t.abs().to(F64).clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(a)) - 7)


def ulps(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """bf16 units in the last place between two bf16 tensors (tests/util.py: bf16_ulps, restated so this module stays
    importable without the package; test_rowops_refs.py checks the two agree)"""
    ai = a.to(BF).view(torch.int16).to(torch.int32)
    bi = b.to(BF).view(torch.int16).to(torch.int32)
    ai = torch.where(ai < 0, -(ai & 0x7fff), ai)
    bi = torch.where(bi < 0, -(bi & 0x7fff), bi)
    return (ai - bi).abs()


def gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(seed)


def randn_bf16(g, *shape, std=1.0, mean=0.0):
    return (torch.randn(*shape, generator=g) * std + mean).to(BF)


# ------------------------------------------------------------------------------------------------ norms
def f32_eps(eps: float) -> float:
    """the kernels take eps as a C float: the references use that very value"""
    return float(torch.tensor(eps, dtype=torch.float32))


def layernorm_ref(x, gamma, beta, eps):
    """nn.LayerNorm on bf16 rows: bf16((x - mean) * rstd * gamma + beta), biased variance, everything before the one rounding
    in fp64.  Returns (bf16 rows, absolute cancellation floor per element, rstd per row, mean per row)."""
    xd, g, b = x.to(F64), gamma.to(F64), beta.to(F64)
    mean = xd.mean(1, keepdim=True)
    var = ((xd - mean) ** 2).mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + f32_eps(eps))
    out = round_bf16((xd - mean) * rstd * g + b)
    floor = FLOOR_REL * xd.abs().amax(1, keepdim=True) * rstd * g.abs()[None, :]
    return out, floor, rstd[:, 0], mean[:, 0]


def rmsnorm_ref(x, w, eps):
    """InternLM2RMSNorm: bf16(w * bf16(x * rsqrt(mean(x^2) + eps))) - TWO rounding points.  Returns (bf16 rows, absolute floor,
    rstd per row, alternatives).  The alternatives are the rows that come out when the FIRST rounding sees x * rstd smaller or
    larger by 2^-20 of itself (an fp32 rstd is that close to the fp64 one, not closer): where x * rstd lies that near a bf16
    rounding boundary, an fp32 implementation may hand the neighbouring bf16 to the gain, and the product is then up to 2 ulps
    from the reference although every operation was correctly rounded (torch's own fp32 formula: 6 of 4.2 M elements at
    1025 x 4096).  Everywhere else the alternatives equal the reference."""
    xd, wd = x.to(F64), w.to(F64)
    rstd = 1.0 / torch.sqrt((xd * xd).mean(1, keepdim=True) + f32_eps(eps))
    h = xd * rstd
    out = round_bf16(wd[None, :] * rb(h))
    alts = [round_bf16(wd[None, :] * rb(h * (1.0 + s * FLOOR_REL))) for s in (-1.0, 1.0)]
    floor = FLOOR_REL * xd.abs().amax(1, keepdim=True) * rstd * wd.abs()[None, :]
    return out, floor, rstd[:, 0], alts


def layernorm_f32(x, gamma, beta, eps):
    """the reference-grade fp32 implementation the kernels are held against: torch's own LayerNorm on fp32 copies"""
    return F.layer_norm(x.float(), (x.shape[1],), gamma.float(), beta.float(), eps).to(BF)


def rmsnorm_f32(x, w, eps):
    """the InternLM2 formula as the reference runs it: fp32 statistics, bf16 product with the gain"""
    h = x.float()
    h = h * torch.rsqrt(h.pow(2).mean(-1, keepdim=True) + eps)
    return w * h.to(BF)


def row_stats_f32(x, eps, mean: bool):
    """fp32 two-pass statistics on the CPU: what an fp32 implementation achieves on these inputs"""
    h = x.float()
    if mean:
        m = h.mean(1, keepdim=True)
        r = torch.rsqrt(((h - m) ** 2).mean(1) + eps)
        return r, m[:, 0] * r
    return torch.rsqrt((h * h).mean(1) + eps), None


def row_stats_ref(x, eps, mean: bool):
    xd = x.to(F64)
    if mean:
        m = xd.mean(1)
        r = 1.0 / torch.sqrt(xd.var(1, unbiased=False) + f32_eps(eps))
        return r, m * r
    return 1.0 / torch.sqrt((xd * xd).mean(1) + f32_eps(eps)), None


def norm_report(out, ref, floor, floor_only=False, alts=()):
    """The bf16-norm rule: an element passes within 1 bf16 ulp of the rounded fp64 reference (or of one of ``alts``, see
    rmsnorm_ref), or within the absolute cancellation floor (``floor_only``: constant and zero rows - the floor alone).
    Returns the figures a test prints; the bit-identical share is always against ``ref``."""
    out, ref = out.cpu(), ref.cpu()
    assert out.shape == ref.shape and out.dtype == BF and ref.dtype == BF, (out.shape, ref.shape, out.dtype)
    u = ulps(out, ref)
    err = (out.to(F64) - ref.to(F64)).abs()
    finite = bool(torch.isfinite(out.float()).all())
    ok = err <= floor
    if not floor_only:
        ok = ok | (u <= 1)
        for a in alts:
            ok = ok | (ulps(out, a) <= 1)
    return dict(finite=finite, bad=int((~ok).sum()), n=ok.numel(), max_ulps=int(u.max()), share=float((u == 0).double().mean()),
                max_err=float(err.max()))


def assert_norm(rep, what, min_share=None):
    assert rep["finite"], f"{what}: non-finite output"
    assert rep["bad"] == 0, f"{what}: {rep['bad']} of {rep['n']} elements outside 1 ulp / the floor (max {rep['max_ulps']} ulps, " \
                            f"max abs err {rep['max_err']:.3e})"
    if min_share is not None:
        assert rep["share"] >= min_share, f"{what}: bit-identical share {rep['share']:.4f} < {min_share:.4f}"


def regime_rows(regime: str, rows: int, dim: int, seed: int) -> torch.Tensor:
    """the value regimes of the norm tests, as bf16 rows"""
    g = gen(seed)
    if regime == "normal":
        return randn_bf16(g, rows, dim)
    if regime == "mean64":        # bf16 steps are 0.5 at 64: a spread of a few steps around a large mean
        return (64.0 + 0.5 * torch.randint(-3, 4, (rows, dim), generator=g)).to(BF)
    if regime == "constant":      # a different non-zero constant per row, var = 0, rstd = eps^-1/2
        c = randn_bf16(g, rows, 1, std=4.0).float()
        c = torch.where(c.abs() < 0.5, torch.full_like(c, 3.140625), c)
        return c.expand(rows, dim).contiguous().to(BF)
    if regime == "zero":
        return torch.zeros(rows, dim, dtype=BF)
    if regime == "massive":       # N(0,1) with one massive activation per row, as the ViT's residual stream has
        x = torch.randn(rows, dim, generator=g)
        col = torch.randint(0, dim, (rows,), generator=g)
        sign = torch.randint(0, 2, (rows,), generator=g).float() * 2 - 1
        x[torch.arange(rows), col] = 3e4 * sign
        return x.to(BF)
    if regime == "tiny":          # eps dominates the variance
        return (torch.randn(rows, dim, generator=g) * 1e-4).to(BF)
    if regime == "alternating":   # +c, -c, +c ... : mean 0 exactly, every |x| equal
        c = randn_bf16(g, rows, 1, std=2.0).float().abs() + 0.25
        s = torch.where(torch.arange(dim) % 2 == 0, 1.0, -1.0)
        return (c * s[None, :]).to(BF)
    raise AssertionError(regime)


def gain_bias(dim: int, seed: int):
    g = gen(seed)
    return randn_bf16(g, dim, std=0.1, mean=1.0), randn_bf16(g, dim, std=0.1)


# ------------------------------------------------------------------------------------------------ layouts
def strided(t: torch.Tensor, ld: int, device, col: int = 0, fill: float = SENTINEL):
    """``t`` [rows, dim] placed at columns [col, col + dim) of a sentinel-filled [rows, ld] buffer on ``device``.
    Returns (buffer, view)."""
    rows, dim = t.shape
    assert col % 8 == 0 and col + dim <= ld
    buf = torch.full((rows, ld), fill, dtype=t.dtype, device=device)
    view = buf[:, col:col + dim]
    view.copy_(t)
    return buf, view


def padding_untouched(buf: torch.Tensor, col: int, dim: int, fill: float = SENTINEL) -> bool:
    """every column of ``buf`` outside [col, col + dim) still holds the sentinel, bit for bit"""
    b = buf.cpu()
    want = torch.full((1,), fill, dtype=b.dtype)
    return bool((b[:, :col] == want).all()) and bool((b[:, col + dim:] == want).all())


def pixel_shuffle_rows(x: torch.Tensor, tiles: int, grid: int) -> torch.Tensor:
    """rows of a [tiles * (1 + grid^2), d] ViT output -> [tiles * (grid/2)^2, 4 d]: output token (tile, a2, b2) is the
    concatenation of source tokens (2a2, 2b2) (2a2, 2b2+1) (2a2+1, 2b2) (2a2+1, 2b2+1), CLS skipped (include/mjv.h)"""
    d = x.shape[1]
    v = x.view(tiles, grid * grid + 1, d)[:, 1:, :].reshape(tiles, grid // 2, 2, grid // 2, 2, d)
    return v.permute(0, 1, 3, 2, 4, 5).reshape(tiles * (grid // 2) ** 2, 4 * d)


# ------------------------------------------------------------------------------------------------ RoPE
def rope_tables(positions: int, rot_dim: int, base: float = 1e6, factor: float = 1.0):
    inv = 1.0 / (base ** (torch.arange(0, rot_dim, 2).float() / rot_dim))
    fr = torch.arange(positions).float()[:, None] * inv[None, :]
    emb = torch.cat((fr, fr), -1)
    return (emb.cos() * factor).to(BF), (emb.sin() * factor).to(BF)


def rope_ref(x, cos, sin):
    """bf16(bf16(x cos) + bf16(rot(x) sin)) on the last dim, fp64 between the rounding points; x [..., D], cos / sin
    broadcastable [..., D]"""
    D = x.shape[-1]
    xd = x.to(F64)
    rot = torch.cat((-xd[..., D // 2:], xd[..., :D // 2]), -1)
    return round_bf16(rb(xd * cos.to(F64)) + rb(rot * sin.to(F64)))


def rope_torch(x, cos, sin):
    """the same formula as elementwise torch bf16 ops (modeling_internlm2.py apply_rotary_pos_emb)"""
    D = x.shape[-1]
    rot = torch.cat((-x[..., D // 2:], x[..., :D // 2]), -1)
    return (x * cos) + (rot * sin)


# ------------------------------------------------------------------------------------------------ reward heads
def heads_case(seed, batch, n_obj, n_asp, groups, hidden, gate_hidden, temperature, regime):
    """Seeded inputs of one reward-heads launch (CPU bf16 tensors + sizes).  ``groups``: list of criteria-id lists in aspect
    order (a partition of range(n_obj), not the identity order).  ``regime``:
      normal  - N(0,1)-like activations and small weights;
      onehot  - every operand a small integer (times a power of two) so that every fp32 sum is exact, one criterion per group
                and one aspect leading by 1024: exp((other - leader) / T) underflows to exactly 0 in fp32 for every T used,
                so the softmaxes are exactly one-hot and every weight is exactly 0 or logit_scale (a lead of 50 would leave
                e^-50 = 1.9e-22, a normal bf16 value whose last bits depend on the exp implementation);
      uniform - the same integer operands with all logits equal: every softmax is 1 / n, one correctly rounded division."""
    g = gen(seed)
    assert sorted(i for grp in groups for i in grp) == list(range(n_obj)) and len(groups) == n_asp
    p = dict(batch=batch, n_obj=n_obj, n_asp=n_asp, hidden=hidden, gate_hidden=gate_hidden, temperature=float(temperature),
             groups=[list(grp) for grp in groups], regime=regime)

    def ints(lo, hi, *shape, scale=1.0):
        return (torch.randint(lo, hi + 1, shape, generator=g).float() * scale).to(BF)

    if regime == "normal":
        p["hr"] = randn_bf16(g, batch, hidden, std=1.1)
        p["ga"] = randn_bf16(g, batch, gate_hidden).clamp_min(0)          # post-ReLU rows
        p["gc"] = randn_bf16(g, batch, gate_hidden).clamp_min(0)
        p["w_reg"] = randn_bf16(g, n_obj, hidden, std=0.05)
        p["w_transform"] = (torch.eye(n_obj) + 0.1 * torch.randn(n_obj, n_obj, generator=g)).to(BF)
        p["wa"], p["ba"] = randn_bf16(g, n_asp, gate_hidden, std=0.05), randn_bf16(g, n_asp, std=0.3)
        p["wc"], p["bc"] = randn_bf16(g, n_obj, gate_hidden, std=0.05), randn_bf16(g, n_obj, std=0.3)
        p["ls_a"], p["ls_c"] = torch.tensor([1.21875], dtype=BF), torch.tensor([0.84375], dtype=BF)
    else:
        # |hr . w_reg| <= hidden * 3 * 2 / 64 = 288 at hidden 3072, a multiple of 2^-6: exact in fp32 in any order
        p["hr"] = ints(-3, 3, batch, hidden)
        p["w_reg"] = ints(-2, 2, n_obj, hidden, scale=2.0 ** -6)
        p["w_transform"] = ints(-2, 2, n_obj, n_obj, scale=0.25)
        p["ga"], p["gc"] = ints(0, 3, batch, gate_hidden), ints(0, 3, batch, gate_hidden)
        p["ls_a"], p["ls_c"] = torch.tensor([1.5], dtype=BF), torch.tensor([0.75], dtype=BF)
        if regime == "onehot":
            # |ga . wa| <= gate_hidden * 3 / 64 <= 48.4: the leader's bias of 1024 keeps it at least 900 ahead
            p["wa"] = ints(-1, 1, n_asp, gate_hidden, scale=2.0 ** -6)
            p["wc"] = ints(-1, 1, n_obj, gate_hidden, scale=2.0 ** -6)
            ba, bc = torch.zeros(n_asp), torch.zeros(n_obj)
            ba[int(torch.randint(0, n_asp, (1,), generator=g))] = 1024.0
            for grp in groups:
                bc[grp[int(torch.randint(0, len(grp), (1,), generator=g))]] = 1024.0
            p["ba"], p["bc"] = ba.to(BF), bc.to(BF)
        elif regime == "uniform":
            p["wa"] = ints(-1, 1, 1, gate_hidden, scale=2.0 ** -6).expand(n_asp, gate_hidden).contiguous()
            p["wc"] = ints(-1, 1, 1, gate_hidden, scale=2.0 ** -6).expand(n_obj, gate_hidden).contiguous()
            p["ba"], p["bc"] = torch.full((n_asp,), 0.5, dtype=BF), torch.full((n_obj,), -2.0, dtype=BF)
        else:
            raise AssertionError(regime)
    return p


def _matvec(a, w, bias=None):
    """fp64 value of a @ w^T (+ bias) before its bf16 rounding, the summed magnitudes, the rounded value, and where the
    rounding is AMBIGUOUS: an fp32 sum in another order (within FLOOR_REL of the summed magnitudes) may round to the
    neighbouring bf16"""
    ad, wd = a.to(F64), w.to(F64)
    v, mag = ad @ wd.t(), ad.abs() @ wd.abs().t()
    if bias is not None:
        v, mag = v + bias.to(F64)[None, :], mag + bias.to(F64).abs()[None, :]
    r = rb(v)
    amb = (rb(v - FLOOR_REL * mag) != r) | (rb(v + FLOOR_REL * mag) != r)
    return v, mag, r, amb


def _softmax_scaled(logits, T, ls):
    """bf16(bf16(softmax(bf16(logits / T))) * logit_scale): the bf16 ops of GatingNetwork.forward (moe_reward.py:34-35)"""
    z = rb(logits / T)
    e = torch.exp(z - z.amax(-1, keepdim=True))
    return rb(rb(e / e.sum(-1, keepdim=True)) * ls)


def heads_ref(p, rewards=None, crit=None, aspect_weights=None, aspect_gating=None):
    """fp64 restatement of heads.hip's comment block / moe_reward.py:239-285 with a bf16 rounding after every torch op.
    ``rewards`` / ``crit`` / ``aspect_weights`` / ``aspect_gating``: the KERNEL's own rounded outputs (bf16 [B, n]); when given,
    everything downstream is computed from them instead, which isolates each stage from a rounding flip in the stage before.
    Returns fp64 tensors plus the summed magnitudes and ambiguity masks the bounds need."""
    T = p["temperature"]
    ls_a, ls_c = float(p["ls_a"][0]), float(p["ls_c"][0])
    o = {}
    v0, mag0, rew0, amb0 = _matvec(p["hr"], p["w_reg"])
    wt = p["w_transform"].to(F64)
    v1 = rew0 @ wt
    o["rewards_mag"] = rew0.abs() @ wt.abs()
    # a flipped first-stage rounding moves rewards[j] by ulp(rew0[k]) * |w_transform[k][j]|
    o["rewards_flip"] = (bf16_ulp(rew0) * amb0.to(F64)) @ wt.abs()
    o["rewards"] = rb(v1)
    _, o["asp_mag"], asp_logit, o["asp_amb"] = _matvec(p["ga"], p["wa"], p["ba"])
    _, o["crit_mag"], o["criteria_gating"], o["crit_amb"] = _matvec(p["gc"], p["wc"], p["bc"])
    rew = o["rewards"] if rewards is None else rewards.to(F64)
    cr = o["criteria_gating"] if crit is None else crit.to(F64)
    o["aspect_gating"] = _softmax_scaled(asp_logit, T, ls_a)
    idx = [i for grp in p["groups"] for i in grp]
    w = torch.cat([_softmax_scaled(cr[:, grp], T, ls_c) for grp in p["groups"]], dim=1)
    o["aspect_weights"] = w
    w_used = w if aspect_weights is None else aspect_weights.to(F64)
    prod = rb(rew[:, idx] * w_used)
    off, scores = 0, []
    for grp in p["groups"]:
        scores.append(rb(prod[:, off:off + len(grp)].sum(1)))
        off += len(grp)
    o["aspect_scores"] = torch.stack(scores, 1)
    ag = o["aspect_gating"] if aspect_gating is None else aspect_gating.to(F64)
    o["score"] = (o["aspect_scores"] * ag).sum(1)
    o["score_mag"] = (o["aspect_scores"] * ag).abs().sum(1)
    o["weighted_last"] = o["aspect_scores"][:, -1]
    return o


@torch.no_grad()
def heads_torch(p):
    """The independent reference: moe_reward.py's order of operations (:239-240 regression + transform, :29-35 last gating
    layer and scaled softmax, :253-277 per-aspect weights, weighted sums, score) as torch bf16 ops on the CPU, entered after
    the gating MLPs' hidden layers - oracle/ref_cpu.py's head math takes the hidden rows and runs those layers itself."""
    T = p["temperature"]
    rewards = F.linear(p["hr"], p["w_reg"]) @ p["w_transform"]
    a = F.linear(p["ga"], p["wa"], p["ba"])
    aspect_gating = F.softmax(a / T, dim=1) * p["ls_a"][0]
    crit = F.linear(p["gc"], p["wc"], p["bc"])
    weights = [F.softmax(crit[:, grp] / T, dim=-1) * p["ls_c"][0] for grp in p["groups"]]
    aspect_scores = torch.zeros(p["batch"], p["n_asp"])
    weighted = None
    for i, grp in enumerate(p["groups"]):
        weighted = (rewards[:, grp] * weights[i]).sum(dim=-1)
        aspect_scores[:, i] = weighted
    score = (aspect_scores * aspect_gating).sum(dim=-1)
    return dict(rewards=rewards, criteria_gating=crit, aspect_gating=aspect_gating, aspect_weights=torch.cat(weights, -1),
                aspect_scores=aspect_scores, score=score, weighted_last=weighted)


def product_groups():
    """28 criteria in 5 aspects, the product's sizes, as a permutation that is not the identity"""
    sizes, order = (6, 5, 7, 4, 6), [(i * 11 + 3) % 28 for i in range(28)]
    out, o = [], 0
    for s in sizes:
        out.append(order[o:o + s])
        o += s
    return out


def strided_groups(n_obj: int, n_asp: int, mult: int):
    """n_asp equal groups over the permutation i -> (i * mult + 1) % n_obj (mult coprime to n_obj)"""
    assert math.gcd(mult, n_obj) == 1 and n_obj % n_asp == 0
    order = [(i * mult + 1) % n_obj for i in range(n_obj)]
    per = n_obj // n_asp
    return [order[a * per:(a + 1) * per] for a in range(n_asp)]
