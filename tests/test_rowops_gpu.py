"""Row kernels (rowops.hip) and the reward heads (heads.hip) on the MI355X against the plain fp64 references of
tests/rowops_ref.py: every template instantiation (IT = 2 / 4 / 8, switching at widths 1024 and 2048), widths with a masked
tail, row counts around the four-rows-per-workgroup edge, strided layouts (padding pre-filled with a sentinel that must survive
bit for bit), the value regimes where a norm goes wrong, and the heads kernel's own parameters through a hand-built HeadsDesc.

Bounds (derived in rowops_ref.py and test_rowops_refs.py, which shows on the CPU that a reference-grade fp32 implementation meets
them): bit-exact for RoPE, patchify, CLS rows, the embedding gather, the MXFP8 norms against norm-then-quantise and the one-hot /
uniform heads cases; bf16 norms within 1 ulp of the rounded fp64 reference or the 2^-20 cancellation floor, with the bit-identical
share held to 0.98 on N(0,1) and to the share torch's fp32 norm reaches on the very same inputs minus 0.01 elsewhere.
"""
import pytest
import torch

import rowops_ref as R
from util import bf16_ulps

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
LAYOUTS = ("contiguous", "pad_in_8", "pad_in_40", "pad_out", "slices")


def _rows_for(dim: int, layout: str) -> int:
    """the pruned cross product: every width meets every layout and, rotating, every row count"""
    return R.NORM_ROWS[(R.NORM_WIDTHS.index(dim) + LAYOUTS.index(layout)) % len(R.NORM_ROWS)]


def _place(x, dim, layout, cuda):
    """input view and sentinel-filled output view of one layout: (x_view, out_buf, out_view, out_col)"""
    rows = x.shape[0]
    if layout == "slices":   # input and output are column slices of ONE wider buffer, at 16-byte-aligned column offsets
        buf, xv = R.strided(x, 2 * dim + 40, cuda, col=8)
        col = dim + 24
        return xv, buf, buf[:, col:col + dim], col
    ldx = dim + {"pad_in_8": 8, "pad_in_40": 40}.get(layout, 0)
    ldy = dim + (40 if layout == "pad_out" else 0)
    _, xv = R.strided(x, ldx, cuda)
    out_buf = torch.full((rows, ldy), R.SENTINEL, dtype=BF, device=cuda)
    return xv, out_buf, out_buf[:, :dim], 0


def _out_padding_untouched(out_buf, col, dim, layout, x):
    b = out_buf.cpu()
    if layout == "slices":   # [sentinel 8 | x | sentinel 16 | out | sentinel 16]
        s = torch.full((1,), R.SENTINEL, dtype=BF)
        return bool((b[:, :8] == s).all() and (b[:, 8 + dim:col] == s).all() and (b[:, col + dim:] == s).all()
                    and torch.equal(b[:, 8:8 + dim], x))
    return R.padding_untouched(out_buf, col, dim)


# ------------------------------------------------------------------------------------------------ norms: widths, rows, strides
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dim", R.NORM_WIDTHS)
def test_layernorm_widths_rows_strides(cuda, dim, layout):
    """layernorm_kernel<2 / 4 / 8> on N(0,1) rows: <= 1 bf16 ulp of the rounded fp64 reference or the cancellation floor,
    >= 0.98 bit-identical, padding bit-unchanged.  (torch's fp32 LayerNorm reaches 0.99997 - 1.0 against the same reference.)"""
    from mj_video_amd import ops
    rows = _rows_for(dim, layout)
    x = R.regime_rows("normal", rows, dim, seed=dim + rows)
    g, b = R.gain_bias(dim, dim + 1)
    xv, out_buf, out, col = _place(x, dim, layout, cuda)
    ops.layernorm(xv, g.to(cuda), b.to(cuda), out, 1e-6)
    torch.cuda.synchronize()
    ref, floor, _, _ = R.layernorm_ref(x, g, b, 1e-6)
    rep = R.norm_report(out, ref, floor)
    print(f"layernorm {rows} x {dim} {layout}: {rep}")
    R.assert_norm(rep, f"layernorm {rows} x {dim} {layout}", 0.98)
    assert _out_padding_untouched(out_buf, col, dim, layout, x), "layernorm wrote outside its rows"


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dim", R.NORM_WIDTHS)
def test_rmsnorm_widths_rows_strides(cuda, dim, layout):
    """rmsnorm_kernel<2 / 4 / 8>, plain and with a row gather (repeats, first and last source row): same rule as LayerNorm, with
    the two-rounding-point alternatives of rowops_ref.rmsnorm_ref.  (The fp32 formula on the CPU reaches 0.99999 - 1.0.)"""
    from mj_video_amd import ops
    rows = _rows_for(dim, layout)
    x = R.regime_rows("normal", rows, dim, seed=dim + rows + 1)
    w, _ = R.gain_bias(dim, dim + 2)
    xv, out_buf, out, col = _place(x, dim, layout, cuda)
    ops.rmsnorm(xv, w.to(cuda), out, 1e-5)
    torch.cuda.synchronize()
    ref, floor, _, alts = R.rmsnorm_ref(x, w, 1e-5)
    rep = R.norm_report(out, ref, floor, alts=alts)
    print(f"rmsnorm {rows} x {dim} {layout}: {rep}")
    R.assert_norm(rep, f"rmsnorm {rows} x {dim} {layout}", 0.98)
    assert _out_padding_untouched(out_buf, col, dim, layout, x), "rmsnorm wrote outside its rows"
    # the gather: more source rows than output rows, an index with repeats that reaches row 0 and the last row
    src = R.regime_rows("normal", rows + 6, dim, seed=dim + rows + 2)
    idx = torch.randint(0, rows + 6, (rows,), generator=R.gen(dim))
    idx[0], idx[-1] = rows + 5, 0
    if rows > 2:
        idx[1] = rows + 5
    sv, out_buf, out, col = _place(src, dim, layout, cuda)
    out_buf, out = out_buf[:rows], out[:rows]
    ops.rmsnorm(sv, w.to(cuda), out, 1e-5, row_index=idx.to(torch.int32).to(cuda))
    torch.cuda.synchronize()
    ref, floor, _, alts = R.rmsnorm_ref(src[idx], w, 1e-5)
    rep = R.norm_report(out, ref, floor, alts=alts)
    print(f"rmsnorm gather {rows} x {dim} {layout}: {rep}")
    R.assert_norm(rep, f"rmsnorm gather {rows} x {dim} {layout}", 0.98)
    if layout != "slices":
        assert R.padding_untouched(out_buf, col, dim)


def _check_row_stats(ops, cuda, x, xv, regime, what):
    """both forms of row_stats on the rows of ``x`` (device view ``xv``).  N(0,1): the tolerances of test_row_stats (rstd rtol
    2e-6; mean * rstd rtol 2e-5 / atol 1e-6).  Other regimes: 4 x the error an fp32 two-pass computation on the CPU has on the
    same rows - never less than 4 x 2^-24, half an fp32 ulp, which no fp32 result is closer than except by luck."""
    rows = x.shape[0]
    n = ops.padded_rows(rows)
    worst = {}
    for mean, eps in ((True, 1e-6), (False, 1e-5)):
        rstd = torch.full((n,), R.SENTINEL, dtype=torch.float32, device=cuda)
        mrs = torch.full((n,), R.SENTINEL, dtype=torch.float32, device=cuda) if mean else None
        ops.row_stats(xv, rstd, mrs, eps)
        torch.cuda.synchronize()
        r64, m64 = R.row_stats_ref(x, eps, mean)
        r32, m32 = R.row_stats_f32(x, eps, mean)
        got = rstd[:rows].cpu().double()
        assert torch.isfinite(got).all(), what
        rel = ((got - r64).abs() / r64).max().item()
        cpu_rel = ((r32.double() - r64).abs() / r64).max().item()
        worst["ln" if mean else "rms"] = (rel, cpu_rel)
        if regime == "normal":
            assert torch.allclose(got, r64, rtol=2e-6, atol=0), (what, rel)
        else:
            assert rel <= 4 * max(cpu_rel, R.FP32_HALF_ULP), (what, mean, rel, cpu_rel)
        assert (rstd[rows:] == R.SENTINEL).all(), f"{what}: rstd written past the rows"
        if mean:
            gm = mrs[:rows].cpu().double()
            if regime == "normal":
                assert torch.allclose(gm, m64, rtol=2e-5, atol=1e-6), what
            else:
                err, cpu_err = (gm - m64).abs().max().item(), (m32.double() - m64).abs().max().item()
                assert err <= 4 * max(cpu_err, R.FP32_HALF_ULP * m64.abs().max().item()), (what, err, cpu_err)
            assert (mrs[rows:] == R.SENTINEL).all()
    print(f"row_stats {what}: rstd max rel err (kernel, fp32 two-pass on the CPU) {worst}")


@pytest.mark.parametrize("layout", ["contiguous", "pad_in_8", "pad_in_40"])
@pytest.mark.parametrize("dim", R.NORM_WIDTHS)
def test_row_stats_widths_rows_strides(cuda, dim, layout):
    """row_stats_kernel<2 / 4 / 8, MEAN / no MEAN> on N(0,1) rows (an fp32 two-pass computation on the CPU: rstd within 1.7e-7)."""
    from mj_video_amd import ops
    rows = _rows_for(dim, layout)
    x = R.regime_rows("normal", rows, dim, seed=dim + rows + 3)
    xv = _place(x, dim, layout, cuda)[0]
    _check_row_stats(ops, cuda, x, xv, "normal", f"{rows} x {dim} {layout}")


# ------------------------------------------------------------------------------------------------ norms: value regimes
@pytest.mark.parametrize("regime", R.REGIMES)
@pytest.mark.parametrize("dim", R.REGIME_WIDTHS)
def test_norm_value_regimes(cuda, dim, regime):
    """LayerNorm, RMSNorm and row_stats where a norm goes wrong: a large mean against a small spread (a one-pass variance loses
    it), constant rows (var = 0), zero rows, one massive activation, eps-dominated rows, alternating +-c.  130 rows, input and
    output padded.  Bit-identical share: N(0,1) 0.98; elsewhere what torch's fp32 norm reaches on the same rows minus 0.01
    (both printed); constant and zero rows by the absolute floor alone.
    The shares the kernel is held against, measured on the CPU (torch fp32 against the fp64 reference, smallest over the four
    widths) - LayerNorm: normal 0.99998, mean64 0.9966, massive 0.9999, tiny 0.9999, alternating 0.9955; RMSNorm: 0.99999 - 1.0
    in every regime; constant and zero rows bit-identical.  fp32 two-pass rstd on the CPU: 4.2e-8 .. 2.0e-7 relative."""
    from mj_video_amd import ops
    rows = 130
    x = R.regime_rows(regime, rows, dim, seed=dim + 7)
    g, b = R.gain_bias(dim, dim + 1)
    flat = regime in ("constant", "zero")
    _, xv = R.strided(x, dim + 8, cuda)
    out_buf = torch.full((rows, dim + 40), R.SENTINEL, dtype=BF, device=cuda)
    out = out_buf[:, :dim]
    ops.layernorm(xv, g.to(cuda), b.to(cuda), out, 1e-6)
    torch.cuda.synchronize()
    ref, floor, _, _ = R.layernorm_ref(x, g, b, 1e-6)
    rep = R.norm_report(out, ref, floor, floor_only=flat)
    cpu = R.norm_report(R.layernorm_f32(x, g, b, 1e-6), ref, floor, floor_only=flat)
    print(f"layernorm {regime} x {dim}: kernel {rep}; fp32 torch share {cpu['share']:.4f}")
    R.assert_norm(rep, f"layernorm {regime} x {dim}", None if flat else (0.98 if regime == "normal" else cpu["share"] - 0.01))
    assert R.padding_untouched(out_buf, 0, dim)
    out_buf.fill_(R.SENTINEL)
    ops.rmsnorm(xv, g.to(cuda), out, 1e-5)
    torch.cuda.synchronize()
    ref, floor, _, alts = R.rmsnorm_ref(x, g, 1e-5)
    rep = R.norm_report(out, ref, floor, floor_only=flat, alts=alts)
    cpu = R.norm_report(R.rmsnorm_f32(x, g, 1e-5), ref, floor, floor_only=flat, alts=alts)
    print(f"rmsnorm {regime} x {dim}: kernel {rep}; fp32 torch share {cpu['share']:.4f}")
    R.assert_norm(rep, f"rmsnorm {regime} x {dim}", None if flat else (0.98 if regime == "normal" else cpu["share"] - 0.01))
    assert R.padding_untouched(out_buf, 0, dim)
    _check_row_stats(ops, cuda, x, xv, regime, f"{regime} x {dim}")


# ------------------------------------------------------------------------------------------------ pixel-shuffle LayerNorm
@pytest.mark.parametrize("grid,d,ldx", [(32, 1024, 1024), (32, 1024, 1064), (16, 1024, 1024), (16, 1024, 1032), (2, 1024, 1024),
                                        (2, 32, 40), (8, 256, 256)])
def test_layernorm_pixel_shuffle_production_shapes(cuda, grid, d, ldx):
    """the gather of the projector's LayerNorm at the production shapes: grid 32 (448^2) and 16 (224^2) with d = 1024 - width
    4096, IT = 8, 1025 / 257 source rows per tile -, 3 tiles, dense and padded source rows; grid 2 is the smallest.  The four
    source rows of an output token differ, so any mix-up of them shows."""
    from mj_video_amd import ops
    tiles = 3
    x = R.regime_rows("normal", tiles * (grid * grid + 1), d, seed=grid + d)
    g, b = R.gain_bias(4 * d, d + 1)
    xbuf, xv = R.strided(x, ldx, cuda)
    orows = tiles * (grid // 2) ** 2
    out_buf = torch.full((orows + 1, 4 * d + 8), R.SENTINEL, dtype=BF, device=cuda)
    out = out_buf[:orows, :4 * d]
    ops.layernorm(xv, g.to(cuda), b.to(cuda), out, 1e-5, gather_grid=grid)
    torch.cuda.synchronize()
    ref, floor, _, _ = R.layernorm_ref(R.pixel_shuffle_rows(x, tiles, grid), g, b, 1e-5)
    rep = R.norm_report(out, ref, floor)
    print(f"layernorm_pixshuf grid {grid} d {d} ldx {ldx}: {rep}")
    R.assert_norm(rep, f"layernorm_pixshuf grid {grid}", 0.98)
    assert R.padding_untouched(out_buf[:orows], 0, 4 * d) and (out_buf[orows] == R.SENTINEL).all()
    assert R.padding_untouched(xbuf, 0, d) and torch.equal(xv.cpu(), x)


# ------------------------------------------------------------------------------------------------ MXFP8 norms
MX_ROWS, MX_WIDTHS = (1, 63, 64, 65, 129), (128, 384, 1152, 3072, 4096)


def _mx_buffers(rows, dim, ldy, cuda):
    """an MX8 whose elements are a view of a sentinel-filled [rows, ldy] byte buffer, scale records pre-filled too"""
    from mj_video_amd import ops
    buf = torch.full((rows, ldy), 0xA5, dtype=torch.uint8, device=cuda)
    scales = torch.full((ops.mxfp8_scale_bytes(rows, dim),), 0xA5, dtype=torch.uint8, device=cuda)
    return buf, ops.MX8(buf[:, :dim], scales)


def _check_mx_norms(cuda, x, g, b, ldx_pad, ldy_pad, what):
    from mj_video_amd import ops
    rows, dim = x.shape
    _, xv = R.strided(x, dim + ldx_pad, cuda)
    gc, bc = g.to(cuda), b.to(cuda)
    for name in ("layernorm", "rmsnorm"):
        ref = torch.empty(rows, dim, dtype=BF, device=cuda)
        buf, out = _mx_buffers(rows, dim, dim + ldy_pad, cuda)
        _, want = _mx_buffers(rows, dim, dim, cuda)
        if name == "layernorm":
            ops.layernorm(xv, gc, bc, ref, 1e-6)
            ops.layernorm_mxfp8(xv, gc, bc, out, 1e-6)
        else:
            ops.rmsnorm(xv, gc, ref, 1e-5)
            ops.rmsnorm_mxfp8(xv, gc, out, 1e-5)
        ops.quantize_mxfp8(ref, want)
        torch.cuda.synchronize()
        assert torch.equal(out.data, want.data), f"{name}_mxfp8 {what}: {int((out.data != want.data).sum())} e4m3 elements differ"
        # both scale buffers started from the same fill: equal everywhere = the same bytes written, to the same records
        assert torch.equal(out.scales, want.scales), f"{name}_mxfp8 {what}: scale records differ"
        assert (buf[:, dim:] == 0xA5).all(), f"{name}_mxfp8 {what}: padding bytes written"


@pytest.mark.parametrize("rows", MX_ROWS)
@pytest.mark.parametrize("dim", MX_WIDTHS)
def test_norms_mxfp8_rows_widths_strides(cuda, rows, dim):
    """layernorm_mxfp8 / rmsnorm_mxfp8 bit-equal to the bf16 norm followed by quantize_mxfp8 at the row counts around a 64-row
    scale group (records are laid out by ceil(rows / 64)), with padded ldx and ldy"""
    i = MX_ROWS.index(rows) + MX_WIDTHS.index(dim)
    x = R.regime_rows("normal", rows, dim, seed=rows + dim)
    g, b = R.gain_bias(dim, dim + 1)
    _check_mx_norms(cuda, x, g, b, (0, 8, 40)[i % 3], (0, 8, 48)[(i // 3) % 3], f"{rows} x {dim}")


@pytest.mark.parametrize("regime", R.REGIMES)
@pytest.mark.parametrize("dim", [1152, 4096])
def test_norms_mxfp8_value_regimes(cuda, dim, regime):
    """the same bit-equality in the value regimes - the massive activation sets the scale of its 32-element block"""
    x = R.regime_rows(regime, 65, dim, seed=dim + 11)
    g, b = R.gain_bias(dim, dim + 1)
    _check_mx_norms(cuda, x, g, b, 8, 8, f"{regime} x {dim}")


# ------------------------------------------------------------------------------------------------ RoPE
def _positions(rows, table_rows, seed):
    pos = torch.randint(0, table_rows, (rows,), generator=R.gen(seed))
    pos[0] = table_rows - 1                      # the table's last row
    if rows > 2:
        pos[1], pos[2] = 0, 0                    # position 0, repeated
    if rows > 4:
        pos[-1] = pos[3]
    return pos


@pytest.mark.parametrize("KV,G,rows", [(1, 0, 31), (1, 1, 2186), (1, 2, 1), (1, 4, 31), (2, 0, 1), (2, 1, 31), (2, 2, 2186), (2, 4, 1),
                                       (8, 0, 2186), (8, 1, 1), (8, 2, 2186), (8, 2, 31), (8, 4, 31)])
def test_rope_split_groups_rows_strides(cuda, KV, G, rows):
    """rope_split with qkv a column slice of a wider buffer and padded q / k: bit-exact against the bf16 formula (and the fp64
    restatement of it); the source - V columns included - and all padding stay untouched.  G = 0: a [k | v] projection, no q."""
    from mj_video_amd import ops
    D, P = 128, 300
    width = KV * (G + 2) * D
    qkv = R.randn_bf16(R.gen(KV * 10 + G + rows), rows, width, std=2.0)
    cos, sin = R.rope_tables(P, D)
    pos = _positions(rows, P, rows + G)
    qkv_buf, qkv_v = R.strided(qkv, width + 24, cuda, col=8)
    q_buf = torch.full((rows, KV * G * D + 8), R.SENTINEL, dtype=BF, device=cuda) if G else None
    k_buf = torch.full((rows, KV * D + 40), R.SENTINEL, dtype=BF, device=cuda)
    q = q_buf[:, :KV * G * D] if G else None
    ops.rope_split(qkv_v, q, k_buf[:, :KV * D], cos.to(cuda), sin.to(cuda), pos.to(torch.int32).to(cuda), KV, G)
    torch.cuda.synchronize()
    t = qkv.view(rows, KV, G + 2, D)
    c, s = cos[pos][:, None, None, :], sin[pos][:, None, None, :]
    want = R.rope_torch(t[:, :, :G + 1], c, s)
    assert torch.equal(want, R.rope_ref(t[:, :, :G + 1], c, s))
    assert torch.equal(k_buf[:, :KV * D].cpu(), want[:, :, G].reshape(rows, -1)), "k"
    assert R.padding_untouched(k_buf, 0, KV * D)
    if G:
        assert torch.equal(q.cpu(), want[:, :, :G].reshape(rows, -1)), "q"
        assert R.padding_untouched(q_buf, 0, KV * G * D)
    assert R.padding_untouched(qkv_buf, 8, width) and torch.equal(qkv_v.cpu(), qkv), "rope_split wrote to its source"


@pytest.mark.parametrize("stride,rot,H,KV,rows", [(96, 96, 4, 2, 77), (96, 48, 4, 2, 77), (96, 32, 32, 32, 5), (128, 128, 4, 1, 77),
                                                  (128, 64, 3, 3, 1), (96, 96, 1, 1, 2186)])
def test_rope_heads_strides_and_partial_rotation(cuda, stride, rot, H, KV, rows):
    """rope_heads in place on the q + k heads of a [q | k | v] row with a padded row stride: bit-exact; the v heads, the
    unrotated tail of every head and the padding stay untouched.  rot_dim < head stride separates the two strides."""
    from mj_video_amd import ops
    P = 200
    width = (H + 2 * KV) * stride
    x = R.randn_bf16(R.gen(stride + rot + rows), rows, width, std=2.0)
    cos, sin = R.rope_tables(P, rot, 1e4, 1.19)
    pos = _positions(rows, P, rows + rot)
    buf, xv = R.strided(x, width + 40, cuda)
    ops.rope_heads(xv, H + KV, stride, cos.to(cuda), sin.to(cuda), pos.to(torch.int32).to(cuda))
    torch.cuda.synchronize()
    t = x[:, :(H + KV) * stride].view(rows, H + KV, stride)
    c, s = cos[pos][:, None, :], sin[pos][:, None, :]
    want = t.clone()
    want[..., :rot] = R.rope_torch(t[..., :rot], c, s)
    assert torch.equal(want[..., :rot], R.rope_ref(t[..., :rot], c, s))
    got = xv.cpu()
    assert torch.equal(got[:, :(H + KV) * stride].view(rows, H + KV, stride), want), "rotated heads"
    assert torch.equal(got[:, (H + KV) * stride:], x[:, (H + KV) * stride:]), "v heads"
    assert R.padding_untouched(buf, 0, width)


# ------------------------------------------------------------------------------------------------ patchify, CLS rows, gather
@pytest.mark.parametrize("S", [224, 448])
@pytest.mark.parametrize("ldp", [588, 592, 640])
def test_patchify_production_shapes(cuda, S, ldp):
    """patch 14 at 224 and 448; columns 588 .. ldp are the zero padding the patch-embedding GEMM's K needs (written by the
    kernel, include/mjv.h), the row after the last patch stays untouched"""
    import torch.nn.functional as F
    from mj_video_amd import ops
    tiles, P = 2, 14
    n = tiles * (S // P) ** 2
    px = R.randn_bf16(R.gen(S + ldp), tiles, 3, S, S)
    buf = torch.full((n + 1, ldp), R.SENTINEL, dtype=BF, device=cuda)
    ops.patchify(px.to(cuda), buf[:n], P)
    torch.cuda.synchronize()
    ref = F.unfold(px.float(), kernel_size=P, stride=P).transpose(1, 2).reshape(n, 3 * P * P).to(BF)
    got = buf.cpu()
    assert torch.equal(got[:n, :588], ref)
    assert (got[:n, 588:] == 0).all() and (got[n] == R.SENTINEL).all()


@pytest.mark.parametrize("dim,ld,tiles,tpt", [(200, 208, 3, 5), (1000, 1024, 2, 1025), (8, 8, 1, 1), (1024, 1064, 4, 257)])
def test_cls_rows_widths_and_strides(cuda, dim, ld, tiles, tpt):
    """widths that are not a multiple of the 256-thread step, ldx > dim: bf16(cls + pos0) in every tile's first row, nothing else"""
    from mj_video_amd import ops
    cls, p0 = R.randn_bf16(R.gen(dim), dim), R.randn_bf16(R.gen(dim + 1), dim)
    buf = torch.full((tiles * tpt + 1, ld), R.SENTINEL, dtype=BF, device=cuda)
    ops.cls_rows(buf[:tiles * tpt, :dim], cls.to(cuda), p0.to(cuda), tiles, tpt)
    torch.cuda.synchronize()
    want = torch.full((tiles * tpt + 1, ld), R.SENTINEL, dtype=BF)
    want[0:tiles * tpt:tpt, :dim] = cls + p0
    assert torch.equal(want[0, :dim], R.round_bf16(cls.double() + p0.double()))
    assert torch.equal(buf.cpu(), want)


@pytest.mark.parametrize("dim,vocab,rows", [(8, 5, 9), (3072, 700, 40), (520, 1000, 1), (2048, 64, 300)])
def test_embed_gather_strides_and_skips(cuda, dim, vocab, rows):
    """padded table and padded output; ids reach 0 and vocab - 1; skipped rows keep their sentinel - also when every id is skip_id"""
    from mj_video_amd import ops
    table = R.randn_bf16(R.gen(dim + vocab), vocab, dim)
    skip = vocab // 2
    ids = torch.randint(0, vocab, (rows,), generator=R.gen(rows))
    ids[0] = vocab - 1
    if rows > 3:
        ids[1], ids[2], ids[3] = 0, skip, skip
    _, tv = R.strided(table, dim + 40, cuda, col=8)
    for these in (ids, torch.full((rows,), skip)):
        buf = torch.full((rows + 1, dim + 8), R.SENTINEL, dtype=BF, device=cuda)
        ops.embed_gather(these.to(torch.int32).to(cuda), tv, buf[:rows, :dim], skip)
        torch.cuda.synchronize()
        want = torch.full((rows + 1, dim + 8), R.SENTINEL, dtype=BF)
        keep = these != skip
        want[:rows, :dim][keep] = table[these[keep]]
        assert torch.equal(buf.cpu(), want)


# ------------------------------------------------------------------------------------------------ alignment refusals
def test_norms_refuse_misaligned_pointers(cuda):
    """every norm moves 16-byte pieces of a row: a base pointer 8 bytes off (a view starting 4 elements in, row strides still
    multiples of 8) is refused on the host before anything is launched, as rope_heads already does"""
    from mj_video_amd import ops
    from mj_video_amd._lib import MjvLibraryError
    rows, dim = 4, 128
    wide = torch.zeros(rows, dim + 8, dtype=BF, device=cuda)
    good, off = wide[:, :dim], wide[:, 4:4 + dim]
    vec = torch.ones(dim + 8, dtype=BF, device=cuda)
    g, g_off = vec[:dim], vec[4:4 + dim]
    out = torch.full((rows, dim + 8), R.SENTINEL, dtype=BF, device=cuda)
    rstd = torch.full((ops.padded_rows(rows),), R.SENTINEL, dtype=torch.float32, device=cuda)
    mx = ops.MX8.empty(rows, dim, cuda)
    calls = {
        "layernorm x": lambda: ops.layernorm(off, g, g, out[:, :dim], 1e-6),
        "layernorm y": lambda: ops.layernorm(good, g, g, out[:, 4:4 + dim], 1e-6),
        "layernorm gamma": lambda: ops.layernorm(good, g_off, g, out[:, :dim], 1e-6),
        "layernorm beta": lambda: ops.layernorm(good, g, g_off, out[:, :dim], 1e-6),
        "rmsnorm x": lambda: ops.rmsnorm(off, g, out[:, :dim], 1e-5),
        "rmsnorm y": lambda: ops.rmsnorm(good, g, out[:, 4:4 + dim], 1e-5),
        "rmsnorm w": lambda: ops.rmsnorm(good, g_off, out[:, :dim], 1e-5),
        "row_stats x": lambda: ops.row_stats(off, rstd, None, 1e-5),
        "layernorm_mxfp8 x": lambda: ops.layernorm_mxfp8(off, g, g, mx, 1e-6),
        "layernorm_mxfp8 gamma": lambda: ops.layernorm_mxfp8(good, g_off, g, mx, 1e-6),
        "rmsnorm_mxfp8 x": lambda: ops.rmsnorm_mxfp8(off, g, mx, 1e-5),
        "rmsnorm_mxfp8 w": lambda: ops.rmsnorm_mxfp8(good, g_off, mx, 1e-5),
    }
    for what, call in calls.items():
        try:
            call()
        except MjvLibraryError as e:
            assert "align" in str(e), (what, str(e))
        else:
            raise AssertionError(f"{what}: a misaligned pointer was accepted")
    torch.cuda.synchronize()
    assert (out == R.SENTINEL).all() and (rstd == R.SENTINEL).all(), "a refused call launched"
    ops.layernorm(good, g, g, out[:, :dim], 1e-6)       # the aligned call still runs
    torch.cuda.synchronize()
    assert (out[:, :dim] == 1.0).all()                  # zero rows: beta


# ------------------------------------------------------------------------------------------------ reward heads
def _run_heads(cuda, p, packed: bool):
    """one ops.reward_heads launch on the case ``p`` through a hand-built HeadsDesc: padded ldh / ldg, every output followed by
    sentinel guard elements.  Returns CPU tensors."""
    from mj_video_amd import ops
    from mj_video_amd._lib import HeadsDesc
    B, n_obj, n_asp = p["batch"], p["n_obj"], p["n_asp"]
    keep = []

    def dev(t):
        keep.append(t.to(cuda).contiguous())
        return keep[-1]

    hr_buf, hr = R.strided(p["hr"], p["hidden"] + 40, cuda)
    hg_buf, hg = R.strided(p["hr"], p["hidden"] + 40, cuda)        # h_g is consumed by the gating GEMMs, not by this kernel
    ga_buf, ga = R.strided(p["ga"], p["gate_hidden"] + 8, cuda)
    gc_buf, gc = R.strided(p["gc"], p["gate_hidden"] + 8, cuda)
    offs, idx = [0], []
    for grp in p["groups"]:
        idx += grp
        offs.append(len(idx))
    d = HeadsDesc()
    d.hr, d.hg, d.ldh, d.hidden = hr.data_ptr(), hg.data_ptr(), hr.stride(0), p["hidden"]
    d.ga, d.gc, d.ldg, d.gate_hidden = ga.data_ptr(), gc.data_ptr(), ga.stride(0), p["gate_hidden"]
    d.w_reg, d.w_transform = dev(p["w_reg"]).data_ptr(), dev(p["w_transform"]).data_ptr()
    d.wa, d.ba, d.wc, d.bc = dev(p["wa"]).data_ptr(), dev(p["ba"]).data_ptr(), dev(p["wc"]).data_ptr(), dev(p["bc"]).data_ptr()
    d.ls_a, d.ls_c = dev(p["ls_a"]).data_ptr(), dev(p["ls_c"]).data_ptr()
    d.temperature = p["temperature"]
    d.batch, d.n_obj, d.n_asp = B, n_obj, n_asp
    d.group_offsets = dev(torch.tensor(offs, dtype=torch.int32)).data_ptr()
    d.group_index = dev(torch.tensor(idx, dtype=torch.int32)).data_ptr()
    GUARD = 64
    shapes = dict(rewards=(n_obj, BF), criteria_gating=(n_obj, BF), aspect_gating=(n_asp, BF), aspect_weights=(n_obj, BF),
                  weighted_last=(1, BF), aspect_scores=(n_asp, torch.float32), score=(1, torch.float32))
    if packed:
        shapes["packed34"] = (1 + n_asp + n_obj, torch.float32)
    outs = {k: torch.full((B * n + GUARD,), R.SENTINEL, dtype=dt, device=cuda) for k, (n, dt) in shapes.items()}
    for k, t in outs.items():
        setattr(d, k, t.data_ptr())
    ops.reward_heads(d, cuda)
    torch.cuda.synchronize()
    res = {}
    for k, (n, dt) in shapes.items():
        t = outs[k].cpu()
        assert (t[B * n:] == R.SENTINEL).all(), f"heads wrote past the end of {k}"
        res[k] = t[:B * n].view(B, n)
    for buf, width in ((hr_buf, p["hidden"]), (ga_buf, p["gate_hidden"]), (gc_buf, p["gate_hidden"])):
        assert R.padding_untouched(buf, 0, width)
    for k in ("weighted_last", "score"):
        res[k] = res[k][:, 0]
    return res


def _check_packed(got, p):
    pk = got["packed34"]
    n_asp = p["n_asp"]
    assert torch.equal(pk[:, 0], got["score"]) and torch.equal(pk[:, 1:1 + n_asp], got["aspect_scores"]) \
        and torch.equal(pk[:, 1 + n_asp:], got["rewards"].float()), "packed34 != (score, aspect_scores, float(rewards))"


BF16_FIELDS = ("rewards", "criteria_gating", "aspect_gating", "aspect_weights", "weighted_last")
# (batch, n_obj, n_asp, groups, hidden, gate_hidden, temperature, packed34 given)
HEADS_CASES = [
    (1, 1, 1, [[0]], 8, 8, 1.0, True),
    (5, 5, 5, [[3], [0], [4], [1], [2]], 520, 1032, 0.5, False),
    (300, 28, 5, R.product_groups(), 2048, 1024, 1.0, True),
    (5, 28, 5, R.product_groups(), 3072, 1032, 4.0, False),
    (300, 64, 16, R.strided_groups(64, 16, 5), 3072, 1024, 0.5, True),
    (5, 64, 16, R.strided_groups(64, 16, 3), 520, 8, 4.0, True),
    (300, 64, 1, R.strided_groups(64, 1, 7), 8, 1032, 1.0, False),
    (1, 64, 1, R.strided_groups(64, 1, 5), 2048, 1024, 0.5, True),
    (1, 5, 5, [[4], [3], [2], [1], [0]], 3072, 8, 4.0, False),
    (300, 1, 1, [[0]], 520, 1032, 4.0, True),
]
HEADS_IDS = [f"B{c[0]}-obj{c[1]}-asp{c[2]}-h{c[4]}-g{c[5]}-T{c[6]}-{'packed' if c[7] else 'nopack'}" for c in HEADS_CASES]


@pytest.mark.parametrize("case", HEADS_CASES, ids=HEADS_IDS)
def test_reward_heads_random_logits(cuda, case):
    """reward_heads_kernel on N(0,1)-like operands, its own parameters varied: batch, n_obj / n_asp up to the 64 / 16 maximum,
    singleton groups, a permuted group_index, hidden / gate_hidden that are not multiples of wave_dot's 512-element stride,
    padded ldh / ldg, temperature, packed34 given or null.
      * rewards, criteria_gating (two rounding points: matvec, then transform / bias): <= 2 ulps of the fp64 restatement, or within
        2^-20 of the summed |terms| next to zero.  One addition for rewards: the first-stage matvec is not an output, so where
        ITS rounding is ambiguous (the fp64 value within 2^-20 of its summed |terms| of a bf16 rounding boundary) the kernel may
        hold the neighbouring bf16, which moves rewards[j] by ulp(rew0[k]) * |w_transform[k][j]| - more than 2 ulps of a
        rewards[j] that cancels.  That term, for the ambiguous k only, is added to the floor.
      * aspect_weights: the restatement recomputed from the KERNEL's criteria_gating, <= 1 ulp (isolates the softmax from a
        matvec flip).  aspect_gating: the kernel does not output the aspect logits; a sample none of whose aspect logits is
        ambiguous in the sense above must hold exactly the restatement's logits, and is held to <= 1 ulp; the other samples
        (printed; a handful in 300) to the end-to-end bound.
      * aspect_scores: recomputed from the kernel's rewards and aspect_weights, bit-equal (one bf16 rounding of an fp32 sum of
        bf16 values); weighted_last is its last column; score: recomputed from the kernel's aspect_scores and aspect_gating,
        within 1e-6 of the summed |terms| (fp32 sum order over <= 16 terms; of the |terms|, not of a score that may cancel).
      * end to end against the independent torch bf16 restatement: the bounds of test_reward_heads_kernel_against_oracle
        (2 ulps or 1e-3; fp32 fields 1 % + 2e-3).
    The worst figure of every field is printed."""
    batch, n_obj, n_asp, groups, hidden, gate_hidden, T, packed = case
    p = R.heads_case(41 + batch + n_obj, batch, n_obj, n_asp, groups, hidden, gate_hidden, T, "normal")
    got = _run_heads(cuda, p, packed)
    for k, t in got.items():
        assert torch.isfinite(t.float()).all(), k
    o = R.heads_ref(p)
    worst = {}
    for f, floor in (("criteria_gating", R.FLOOR_REL * o["crit_mag"]),
                     ("rewards", R.FLOOR_REL * o["rewards_mag"] + o["rewards_flip"])):
        u = bf16_ulps(got[f], R.round_bf16(o[f]))
        ok = (u <= 2) | ((got[f].double() - o[f]).abs() <= floor)
        worst[f] = int(u.max())
        assert ok.all(), (f, int(u.max()), int((~ok).sum()))
    own = R.heads_ref(p, rewards=got["rewards"], crit=got["criteria_gating"], aspect_weights=got["aspect_weights"],
                      aspect_gating=got["aspect_gating"])
    u = bf16_ulps(got["aspect_weights"], R.round_bf16(own["aspect_weights"]))
    worst["aspect_weights"] = int(u.max())
    assert int(u.max()) <= 1, ("aspect_weights from the kernel's own criteria_gating", int(u.max()))
    u = bf16_ulps(got["aspect_gating"], R.round_bf16(o["aspect_gating"]))
    sure = ~o["asp_amb"].any(1)
    worst["aspect_gating"] = int(u[sure].max()) if sure.any() else 0
    worst["samples with an ambiguous aspect logit"] = int((~sure).sum())
    assert (u[sure] <= 1).all(), ("aspect_gating", int(u[sure].max()))
    rest = (u <= 2) | ((got["aspect_gating"].double() - o["aspect_gating"]).abs() <= 1e-3)
    assert rest.all(), "aspect_gating, samples with an ambiguous logit"
    assert torch.equal(got["aspect_scores"], own["aspect_scores"].float()), "aspect_scores from the kernel's own rewards and weights"
    assert torch.equal(got["weighted_last"], R.round_bf16(got["aspect_scores"][:, -1].double())), "weighted_last"
    err = (got["score"].double() - own["score"]).abs()
    worst["score / summed |terms|"] = float((err / own["score_mag"].clamp_min(1e-30)).max())
    assert (err <= 1e-6 * own["score_mag"]).all(), ("score", worst)
    t = R.heads_torch(p)
    for f in BF16_FIELDS:
        u = bf16_ulps(got[f], t[f])
        ok = (u <= 2) | ((got[f].float() - t[f].float()).abs() <= 1e-3)
        assert ok.all(), ("end to end", f, int(u.max()))
    for f in ("aspect_scores", "score"):
        e = (got[f] - t[f]).abs()
        assert (e <= 0.01 * t[f].abs() + 2e-3).all(), ("end to end", f, float(e.max()))
    if packed:
        _check_packed(got, p)
    print(f"heads {HEADS_IDS[HEADS_CASES.index(case)]}: worst {worst}")


@pytest.mark.parametrize("regime", ["onehot", "uniform"])
@pytest.mark.parametrize("case", HEADS_CASES, ids=HEADS_IDS)
def test_reward_heads_exact_cases(cuda, case, regime):
    """saturated logits (one criterion per group and one aspect leading by 1024: the softmaxes are exactly one-hot, the weights
    exactly 0 or logit_scale) and all-equal logits (uniform softmax, one correctly rounded 1 / n) on small-integer operands:
    every fp32 sum is exact whatever its order (test_rowops_refs.py: test_exact_heads_cases_are_exact), so every field is
    bit-equal to the fp64 restatement.  The one exception is the uniform case's score, an fp32 sum of up to 16 sixteen-bit
    products of mixed exponents, which is held to 1e-6 of the summed |terms|; the one-hot score has a single non-zero term and
    is bit-equal."""
    batch, n_obj, n_asp, groups, hidden, gate_hidden, T, packed = case
    p = R.heads_case(43 + batch + n_obj, batch, n_obj, n_asp, groups, hidden, gate_hidden, T, regime)
    got = _run_heads(cuda, p, packed)
    o = R.heads_ref(p)
    for f in BF16_FIELDS:
        assert torch.equal(got[f], R.round_bf16(o[f])), (regime, f, int(bf16_ulps(got[f], R.round_bf16(o[f])).max()))
    assert torch.equal(got["aspect_scores"], o["aspect_scores"].float()), (regime, "aspect_scores")
    if regime == "onehot":
        w, ag = got["aspect_weights"].float(), got["aspect_gating"].float()
        assert ((w == 0) | (w == 0.75)).all() and int((w == 0.75).sum()) == batch * n_asp
        assert ((ag == 0) | (ag == 1.5)).all() and int((ag == 1.5).sum()) == batch
        assert torch.equal(got["score"], o["score"].float()), "score"
    else:
        assert ((got["score"].double() - o["score"]).abs() <= 1e-6 * o["score_mag"]).all(), "score"
    if packed:
        _check_packed(got, p)
