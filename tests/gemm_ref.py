"""Exact references of the GEMMs (gemm.hip, gemm_fp8.hip) over operand layouts, row maps and rotary groups, per kernel form:
the case table, operands that make every result exact, the epilogue formulas of include/mjv.h in fp64 with their bf16 rounding
points, the placement of the operands in sentinel-filled buffers, the whole-buffer comparison of test_gemm_layouts_gpu.py, and a
torch emulation of a kernel's addressing with which test_gemm_refs.py shows that the comparison can fail.  Test infrastructure
only: imports torch and rowops_ref, never the library, so everything here runs without a GPU.

Why the results are exact.  A, W, bias and residual hold small integers (MXFP8: integers times per-block powers of two), so with
K * max|a| * max|w| < 2^24 every partial sum of every summation order is an integer (or a multiple of the smallest block scale
product) that fp32 holds exactly: the accumulator is THE value, whichever kernel, K slicing and MFMA order produced it.  LayerScale
comes from {+-1, +-2, +-0.5}, the folded-norm vectors are powers of two (row_scale) and small integers, so each epilogue is a chain
of exact fp32 operations and bf16 roundings of exact values - deterministic.  GELU is the bit-exact table (torch's CPU bf16 GELU,
test_gemm_gelu_is_exact_for_every_bf16_input), the rotary embedding is three bf16 roundings of bf16 x bf16 products.  SiLU-mul is
the one epilogue with a transcendental: it keeps the bound test_gemm_silu_mul states (3 ulps, 0.95 bit-identical, 2e-3).
"""
import zlib

import torch
import torch.nn.functional as F

import rowops_ref as R
from rowops_ref import BF, F64, SENTINEL

SENTINEL_U8 = 0xA5            # what MXFP8 element / scale bytes hold before a launch
ROPE_POSITIONS = 64           # rows of the cos / sin tables
PERIOD = 50                   # row-map period (51 rows out): no divisor of any tile height, straddles every tile edge
SILU_BOUND = dict(max_ulps=3, frac_exact=0.95, atol=2e-3)      # test_gemm_silu_mul

BF16_EPIS = ("bias", "nobias", "gelu", "relu", "scale_res", "res", "silu", "ln_bias", "ln_gelu", "rms_silu")
F8_EPIS = ("bias", "gelu", "relu", "scale_res", "silu", "bias_out8", "gelu_out8", "relu_out8", "silu_out8")
BF16_LAYOUTS = ("contiguous", "pad_a", "pad_w", "pad_c", "res_apart", "slices", "m_short")
F8_LAYOUTS = ("contiguous", "pad_a", "pad_w", "pad_c", "res_apart", "slices")     # (an MXFP8 operand's scale records fix its row count)
RESIDUAL = ("scale_res", "res")
PERSISTENT_EPIS = ("bias", "nobias", "relu", "silu", "ln_bias", "rms_silu")
MUTANTS = ("ldc_width", "ldr_width", "res_mod_relative", "out_group_relative", "out_rows_ignored", "tile_unwritten",
           "cols_past_n", "kv_group_from_tile", "ldq_width")


def _forms(c):
    """form -> (tile, workspace, M, N, K, accepted epilogues, accepted row maps, tile height, tile width).  Each shape is the
    smallest with a ragged last m-tile, a ragged last n-tile and the form's own minimum K; c = compute units of the device."""
    every = BF16_EPIS
    return {
        "skinny64": (64, False, 77, 40, 192, every, ("group", "rows"), 64, 32),
        "t128": (128, False, 141, 136, 192, every, ("group", "rows"), 128, 128),
        "t128_sliced": (128, True, 141, 136, 4160, every, ("group", "rows"), 128, 128),
        "t256": (256, False, 269, 264, 192, every, ("group", "rows"), 256, 256),                 # 3 K-tiles: never persistent
        "t256_persistent": (256, False, 256 * (c // 2) + 13, 264, 256, PERSISTENT_EPIS, ("group", "rows"), 256, 256),   # c + 2 tiles
        "t256_sliced": (0, True, 400, 264, 4096, every, ("group",), 256, 256),
        "two_per_cu": (2, False, 141, 264, 192, ("bias", "nobias", "gelu", "scale_res", "res"), (), 128, 256),
        "peeled_128_tail": (0, False, 256 * c + 141, 264, 64, every, ("group",), 256, 256),
        "peeled_skinny_tail": (0, False, 256 * c + 77, 264, 64, every, ("group",), 256, 256),
        "f8_t256": (256, False, 269, 264, 384, F8_EPIS, (), 256, 256),
        "f8_sliced": (0, True, 269, 264, 1024, F8_EPIS, (), 256, 256),
        "f8_peeled_sliced_tail": (0, True, 2112, 8192, 1024, F8_EPIS, (), 256, 256),
    }


def form_names():
    return tuple(_forms(256))


def form_accepts(form):
    """(epilogues, layouts, row maps) a form takes; a form without a residual epilogue (the persistent kernel) has no res_apart"""
    f = _forms(256)[form]
    layouts = F8_LAYOUTS if form.startswith("f8") else BF16_LAYOUTS
    if not any(e in RESIDUAL for e in f[5]):
        layouts = tuple(x for x in layouts if x != "res_apart")
    return f[5], layouts, f[6]


def _expect(form, c, M, persistent):
    """(launch rows [(row0, rows, family)], plan [(family, sliced, persistent, rope_split_after)], smallest c at which the plan
    is guaranteed) - derived by hand from the rules of gemm_plan.h"""
    one = lambda fam, sl=False, p=0: ([(0, M, fam)], [(fam, sl, p, 0)])
    if form == "skinny64":
        return (*one(64), 0)
    if form == "t128":
        return (*one(128), 0)
    if form == "t128_sliced":
        return (*one(128, True), 8)
    if form == "t256":
        return (*one(256), 0)
    if form == "t256_persistent":
        return (*one(256, False, int(persistent)), 0)
    if form == "t256_sliced":
        return (*one(256, True), 48)
    if form == "two_per_cu":
        return (*one(2), 0)
    if form in ("peeled_128_tail", "peeled_skinny_tail"):
        fam = 128 if form == "peeled_128_tail" else 64
        return [(0, 256 * c, 256), (256 * c, M - 256 * c, fam)], [(256, False, 0, 0), (fam, False, 0, 0)], 2
    if form == "f8_t256":
        return (*one(256), 0)
    if form == "f8_sliced":
        return (*one(256, True), 8)
    if form == "f8_peeled_sliced_tail":    # 9 x 32 = 288 tiles: one round of 256 + 32 -> 64 tail rows, K-sliced (256 CUs only)
        return [(0, 2048, 256), (2048, 64, 256)], [(256, False, 0, 0), (256, True, 0, 0)], -256
    raise AssertionError(form)


def _case(c, form, epi, layout, rowmap=None, **over):
    tile, ws, M, N, K = _forms(c)[form][:5]
    fp8 = form.startswith("f8")
    out8 = epi.endswith("_out8")
    base = epi[:-5] if out8 else epi
    if base in ("silu", "rms_silu"):
        N = 288 if N <= 264 else N                     # 9 pairs of 16 + 16 weight rows: 144 output columns
        if out8:
            N = 768 if N == 288 else N                 # an MXFP8 output's width is a multiple of 128
    elif out8 and N == 264:
        N = 384
    case = dict(form=form, epi=base, out8=out8, fp8=fp8, layout=layout, rowmap=rowmap, tile=tile, ws=ws, M=M, N=N, K=K,
                rope_group=None, rope_place=None, refuse=False, cus=c)
    case.update(over)
    M = case["M"]
    launches, plan, min_cus = _expect(form, c, M, base in PERSISTENT_EPIS)
    if rowmap == "rows" and form in ("t256_sliced", "peeled_128_tail", "peeled_skinny_tail"):
        # out_rows: no peeled tail and no K-sliced 256 tiles (gemm_plan.h).  The peeled shapes then run as ONE unsliced 256-tile
        # launch; t256_sliced's 400 rows fall to the 128-tile kernel, which slices K through the same workspace
        launches, plan, min_cus = ([(0, M, 128)], [(128, True, 0, 0)], 16) if form == "t256_sliced" else ([(0, M, 256)], [(256, False, 0, 0)], 0)
    if case["rope_group"] is not None:
        # only the unsliced 256-tile kernel has the rotary epilogue; every other launch stores the un-rotated heads and the
        # rotary step follows (the plan's rope_split_after)
        plan = [(f, s, p, int(f != 256)) for f, s, p, _ in plan]
    case.update(launches=launches, plan=plan, min_cus=min_cus)
    case["name"] = "-".join(str(x) for x in (form, epi if case["rope_group"] is None else f"rope{case['rope_group']}{case['rope_place']}",
                                              layout, rowmap or "plain") if x)
    if case["refuse"]:
        case["name"] += "-refused"
    case["seed"] = zlib.crc32(case["name"].encode()) & 0x7FFFFFFF
    return case


def cases(cus: int):
    """the whole matrix as plain dicts; epilogues rotate over forms and layouts so that every (form, epilogue), (form, layout) and
    (form, row map) pair occurs (test_gemm_refs.py asserts it)"""
    out, seen = [], set()

    def add(case):
        if case["name"] not in seen:
            seen.add(case["name"])
            out.append(case)

    for fi, form in enumerate(_forms(cus)):
        epis, layouts, maps = form_accepts(form)
        res_epis = [e for e in epis if e in RESIDUAL]
        for i in range(max(len(epis), len(layouts))):
            epi, layout = epis[(i + fi) % len(epis)], layouts[i % len(layouts)]
            if layout == "res_apart" and epi not in RESIDUAL:      # (a residual of its own needs a residual epilogue)
                add(_case(cus, form, epi, "contiguous"))
                epi = res_epis[fi % len(res_epis)]
            add(_case(cus, form, epi, layout))
        # row maps: the patch-embedding pair (LayerScale-free bias + pos-emb residual through res_mod, one CLS slot per period) and
        # the <IMG_CONTEXT> splice; the persistent form has no residual epilogue, so its period map is out_group / out_pad alone
        for m in maps:
            if m == "group":
                add(_case(cus, form, "bias" if form == "t256_persistent" else "scale_res", ("res_apart", "pad_c", "contiguous")[fi % 3]
                          if form != "t256_persistent" else "pad_c", "group"))
            else:
                add(_case(cus, form, [e for e in ("bias", "relu", "gelu", "nobias") if e in epis][fi % 3], ("pad_c", "contiguous", "slices")[fi % 3], "rows"))
    # out_rows on the shapes of the K-sliced 256 form and the peeled forms: the plan falls back to one launch
    for form in ("t256_sliced", "peeled_128_tail", "peeled_skinny_tail"):
        add(_case(cus, form, "bias", "pad_c", "rows"))
    # tile 2 and MXFP8 operands refuse every row map
    for form in ("two_per_cu", "f8_t256"):
        for m in ("group", "rows", "res_mod"):
            add(_case(cus, form, "scale_res" if m != "rows" else "bias", "contiguous", m, refuse=True))
    # rotary epilogue: hidden 192, two kv groups of (g + 2) heads; the 256-tile kernel, then the fallback of the small kernels
    for g in (0, 1, 2, 4):
        N = 2 * (g + 2) * 128
        for place_ in ("contig", "slices"):
            add(_case(cus, "t256", "rope", "pad_c", M=269, N=N, K=192, rope_group=g, rope_place=place_))
        add(_case(cus, "t128", "rope", "pad_c", M=269, N=N, K=192, rope_group=g, rope_place=("contig", "slices")[g % 2]))
        add(_case(cus, "skinny64", "rope", "pad_c", M=269, N=N, K=192, rope_group=g, rope_place=("slices", "contig")[g % 2]))
    add(_case(cus, "peeled_128_tail", "rope", "pad_c", N=512, K=192, rope_group=2, rope_place="slices"))
    return out


# ------------------------------------------------------------------------------------------------ operands
def _ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def operands(case):
    """seeded CPU operands of a case: bf16 values (for MXFP8 cases: values the block quantiser represents exactly)"""
    M, N, K, epi = case["M"], case["N"], case["K"], case["epi"]
    # A and W are seeded by the problem's shape, everything else by the case: the cases of one form share their product
    g = R.gen(zlib.crc32(repr((M, N, K, case["fp8"])).encode()) & 0x7FFFFFFF)
    o = {"aw_key": (M, N, K, case["fp8"])}
    if case["fp8"]:
        # integers times per-block powers of two (tools/fuzz_kernels.py gemm8_case): e4m3 holds |i| <= 8 exactly, the block scale
        # is a power of two, so quantisation is lossless
        a = _ints(g, -8, 8, M, K) * torch.exp2(_ints(g, -1, 1, M, K // 32)).repeat_interleave(32, 1)
        w = _ints(g, -7, 7, N, K) * torch.exp2(_ints(g, -1, 1, N, K // 32)).repeat_interleave(32, 1)
    else:
        a, w = _ints(g, -4, 4, M, K), _ints(g, -3, 3, N, K)
    if K >= 1024:     # deep K thinned as in test_gemm_split_k_matches_unsplit: the sums stay small enough to be bf16 values
        a = a * (torch.rand(M, K, generator=g) < 0.15)
    o["a"], o["w"] = a.to(BF), w.to(BF)
    g = R.gen(case["seed"])
    if epi in ("bias", "gelu", "relu", "scale_res"):
        o["bias"] = _ints(g, -8, 8, N).to(BF)
    if epi == "scale_res" and case["rowmap"] not in ("group", "res_mod"):
        o["scale"] = torch.tensor([1.0, -1.0, 2.0, -2.0, 0.5, -0.5])[torch.randint(0, 6, (N,), generator=g)].to(BF)
    if epi in RESIDUAL:
        rows = PERIOD + 1 if case["rowmap"] in ("group", "res_mod") else M
        o["res"] = _ints(g, -8, 8, rows, N).to(BF)
    if case["rowmap"] == "rows":
        o["out_rows"] = torch.randperm(case["M"] + case["M"] // 4, generator=g)[:M].to(torch.int32)
    pad = lambda n: (n + 255) // 256 * 256         # the 256-tile kernel fetches whole tiles of the fp32 vectors
    if epi in ("ln_bias", "ln_gelu", "rms_silu"):
        rs = torch.zeros(pad(M))
        rs[:M] = torch.exp2(_ints(g, -2, 1, M))
        o["row_scale"] = rs
    if epi in ("ln_bias", "ln_gelu"):
        rsh, csh, bf = torch.zeros(pad(M)), torch.zeros(pad(N)), torch.zeros(pad(N))
        rsh[:M], csh[:N], bf[:N] = _ints(g, -3, 3, M), _ints(g, -4, 4, N), _ints(g, -8, 8, N)
        o.update(row_shift=rsh, col_shift=csh, bias_f32=bf)
    if case["rope_group"] is not None:
        pos = torch.randint(0, ROPE_POSITIONS, (M,), generator=g).to(torch.int32)
        pos[0], pos[1], pos[M - 1] = 0, ROPE_POSITIONS - 1, ROPE_POSITIONS - 1
        o["pos"] = pos
        o["cos"], o["sin"] = R.rope_tables(ROPE_POSITIONS, 128)
    return o


def max_partial_sum(case, o):
    """upper bound of every |partial sum| of the accumulator and of the fp32 epilogue terms, in units of the smallest quantum
    (1 for bf16 integers, 2^-2 for the MXFP8 block-scale products): below 2^24 every fp32 operation before a rounding is exact"""
    quantum = 0.25 if case["fp8"] else 1.0
    acc = float((o["a"].double().abs() @ o["w"].double().abs().t()).max())
    extra = 0.0
    if "row_scale" in o:                                  # row_scale * acc: a power of two times an integer, quantum 2^-2
        acc, quantum = acc * 2.0, 0.25
    if "row_shift" in o:
        extra += float(o["row_shift"].abs().max() * o["col_shift"].abs().max() + o["bias_f32"].abs().max())
    if "bias" in o:
        extra += float(o["bias"].float().abs().max())
    return (acc + extra) / quantum


# ------------------------------------------------------------------------------------------------ the epilogue formulas
_ACC = {}     # the last few products, by (shape key, dtype, order): the cases of a form differ in epilogue and layout only


def _accumulate(o, dtype, device, chunked):
    key = (o["aw_key"], dtype, chunked)
    if key not in _ACC:
        a, w = o["a"], o["w"]
        if not chunked:
            acc = (a.to(device=device, dtype=dtype) @ w.to(device=device, dtype=dtype).t()).cpu()
        else:
            acc = torch.zeros(a.shape[0], w.shape[0], dtype=dtype)
            for k0 in reversed(range(0, a.shape[1], 64)):        # another summation order: 64-wide chunks, last first
                acc = acc + a[:, k0:k0 + 64].to(dtype) @ w[:, k0:k0 + 64].to(dtype).t()
        while len(_ACC) >= 4:
            _ACC.pop(next(iter(_ACC)))
        _ACC[key] = acc
    return _ACC[key]


def values(case, o, dtype=F64, device="cpu", chunked=False, acc=None, res=None):
    """include/mjv.h's epilogue formula on the accumulator, ``dtype`` arithmetic between the bf16 rounding points.  Returns the
    bf16 cells the call writes, [M, output width] (EPI_ROPE_QKV: the bf16 Linear [M, N]).  ``acc``: the accumulator, if the
    caller has it; ``res``: the residual row of every problem row [M, N], if the caller read it itself (emulate)."""
    epi, M = case["epi"], case["M"]
    rb = lambda t: R.round_bf16(t).to(dtype)
    v = _accumulate(o, dtype, device, chunked) if acc is None else acc.to(dtype)
    if "row_scale" in o:
        v = v * o["row_scale"][:M, None].to(dtype)
        if "row_shift" in o:
            N = case["N"]
            v = v + (-o["row_shift"][:M, None].to(dtype) * o["col_shift"][None, :N].to(dtype) + o["bias_f32"][None, :N].to(dtype))
    if "bias" in o:
        v = v + o["bias"].to(dtype)[None, :]
    if epi in ("bias", "nobias", "ln_bias", "rope"):
        return R.round_bf16(v)
    if epi in ("gelu", "ln_gelu"):
        return F.gelu(R.round_bf16(v))                    # torch's CPU bf16 GELU: the table's definition
    if epi == "relu":
        return R.round_bf16(v.clamp_min(0))
    if epi in RESIDUAL:
        v = rb(v)
        if "scale" in o:
            v = rb(v * o["scale"].to(dtype)[None, :])
        if res is None:
            res = o["res"][1 + torch.arange(M) % PERIOD] if case["rowmap"] in ("group", "res_mod") else o["res"]
        return R.round_bf16(res.to(dtype) + v)
    if epi in ("silu", "rms_silu"):
        t = rb(v).view(M, case["N"] // 32, 2, 16)         # W rows interleaved [16 x w1 | 16 x w3]
        gate, up = t[:, :, 0], t[:, :, 1]
        return R.round_bf16(rb(gate / (1.0 + torch.exp(-gate))) * up).reshape(M, case["N"] // 2)
    raise AssertionError(epi)


def silu_fp32_share(case, o):
    """share of SiLU-mul cells an fp32 x * rcp(1 + e^-x) rounds to the fp64 reference's bf16, bit for bit, and the number of cells
    outside SILU_BOUND (more than max_ulps AND more than atol away)"""
    ref = values(case, o)
    t = R.round_bf16(_accumulate(o, torch.float32, "cpu", False) * (o["row_scale"][:case["M"], None] if "row_scale" in o else 1.0))
    t = t.float().view(case["M"], case["N"] // 32, 2, 16)
    gate, up = t[:, :, 0], t[:, :, 1]
    got = ((gate * torch.reciprocal(1.0 + torch.exp(-gate))).to(BF).float() * up).to(BF).reshape(ref.shape)
    u = R.ulps(got, ref)
    beyond = (u > SILU_BOUND["max_ulps"]) & ((got.float() - ref.float()).abs() > SILU_BOUND["atol"])
    return float((u == 0).double().mean()), int(beyond.sum())


# ------------------------------------------------------------------------------------------------ MXFP8 (include/mjv.h)
def mx_quantize(x):
    """bf16 [rows, cols] -> (e4m3 codes uint8 [rows, cols], scale bytes uint8 [rows, cols / 32]): the block quantiser of
    include/mjv.h as oracle/ref_fp8.py states it (b = max(1, E - 8 + (m > 0x60)), element = e4m3_rne(x / 2^(b - 127)))"""
    rows, cols = x.shape
    xb = x.to(BF).reshape(rows, cols // 32, 32)
    u = xb.view(torch.int16).to(torch.int32) & 0x7FFF
    b = (((u.amax(dim=2) + 0x1F) >> 7) - 8).clamp_min(1)
    xf = xb.float()
    codes = torch.ldexp(xf, (127 - b)[:, :, None].expand_as(xf)).to(torch.float8_e4m3fn).view(torch.uint8)
    return codes.reshape(rows, cols), b.to(torch.uint8)


def mx_dequantize(codes, sb):
    rows, cols = codes.shape
    v = codes.view(torch.float8_e4m3fn).float().reshape(rows, cols // 32, 32)
    return torch.ldexp(v, (sb.to(torch.int32) - 127)[:, :, None].expand_as(v)).reshape(rows, cols)


def mx_scale_bytes(rows, cols):
    return (cols // 128) * ((rows + 63) // 64) * 256


def mx_scale_image(sb, fill=SENTINEL_U8):
    """scale bytes [rows, cols / 32] -> the record image of include/mjv.h; bytes of rows behind ``rows`` keep ``fill``"""
    rows, nb = sb.shape
    groups = (rows + 63) // 64
    img = torch.full((nb // 4 * groups * 256,), fill, dtype=torch.uint8)
    r = torch.arange(rows)[:, None]
    blk = torch.arange(nb)[None, :]
    off = ((blk // 4) * groups + r // 64) * 256 + (r % 16) * 16 + (blk % 4) * 4 + (r // 16) % 4
    img[off.reshape(-1)] = sb.reshape(-1)
    return img


# ------------------------------------------------------------------------------------------------ layouts
def out_width(case):
    return case["N"] // 2 if case["epi"] in ("silu", "rms_silu") else case["N"]


def geometry(case):
    """leading dimensions, column offsets and row counts of every operand of a case - all inside the header's contract
    (bf16: multiples of 8 elements, 16-byte aligned offsets; MXFP8 bytes: multiples of 16; an MX8 output: ldc = width + 8)"""
    M, K, lay, W = case["M"], case["K"], case["layout"], out_width(case)
    f8 = case["fp8"]
    g = dict(lda=K, a_col=0, ldw=K, ldc=W, c_col=0, a_rows=M, c_rows=M, res_inplace=case["epi"] in RESIDUAL, ldr=case["N"], r_col=0)
    if lay == "pad_a":
        g["lda"] = K + (16 if f8 else 8)
    elif lay == "pad_w":
        g["ldw"] = K + (48 if f8 else 40)
    elif lay == "pad_c":
        g["ldc"] = W + 8
    elif lay == "res_apart":
        g.update(res_inplace=False, ldr=case["N"] + 40)
    elif lay == "slices":
        g.update(lda=K + (48 if f8 else 24), a_col=16 if f8 else 8, ldc=W + 40, c_col=16, res_inplace=False, ldr=case["N"] + 48, r_col=24)
    elif lay == "m_short":
        g.update(a_rows=M + 5, c_rows=M + 5)
    if case["rowmap"] in ("group", "res_mod"):
        g["res_inplace"] = False
    if case["rowmap"] == "group":
        g["c_rows"] = (M + PERIOD - 1) // PERIOD * (PERIOD + 1)
    if case["rowmap"] == "rows":
        g["c_rows"] = M + M // 4
    if g["res_inplace"]:
        g.update(ldr=g["ldc"], r_col=g["c_col"])
    if case["rope_group"] is not None:
        G = case["rope_group"]
        kv = case["N"] // ((G + 2) * 128)
        qw, kw = kv * G * 128, kv * 128
        if case["rope_place"] == "contig":
            g.update(qw=qw, kw=kw, ldq=qw, q_col=0, ldk=kw, k_col=0)
        else:                  # q and k as column slices of ONE buffer: | 8 | q | 16 | k | 24 |
            g.update(qw=qw, kw=kw, ldq=qw + kw + 48, q_col=8, ldk=qw + kw + 48, k_col=8 + qw + 16)
    return g


def out_rows_of(case, o):
    """output row of every problem row m (absolute), by include/mjv.h's rule"""
    m = torch.arange(case["M"])
    if case["rowmap"] == "rows":
        return o["out_rows"].long()
    if case["rowmap"] == "group":
        return (m // PERIOD) * (PERIOD + 1) + 1 + m % PERIOD
    return m


def place(case, device="cpu", o=None):
    """the operand views of a case's layout inside buffers pre-filled with the sentinel.  Returns dict(a, w, out, kw = keyword
    tensors of the call by ops.gemm's names, bufs = the whole buffer behind every tensor the call may write, o = the operands).
    MXFP8 cases: ``a`` / ``w`` are (bf16 values, uint8 element view, uint8 scale buffer) for ops.quantize_mxfp8 to fill, ``out``
    of an MX8 output is (uint8 element view, uint8 scale buffer)."""
    o = operands(case) if o is None else o
    g = geometry(case)
    M, N, K, W = case["M"], case["N"], case["K"], out_width(case)
    p = dict(o=o, kw={}, bufs={}, g=g)
    if case["fp8"]:
        for key, rows, ld, col in (("a", M, g["lda"], g["a_col"]), ("w", N, g["ldw"], 0)):
            buf = torch.full((rows, ld), SENTINEL_U8, dtype=torch.uint8, device=device)
            sc = torch.full((mx_scale_bytes(rows, K),), SENTINEL_U8, dtype=torch.uint8, device=device)
            p[key] = (o[key].to(device), buf[:, col:col + K], sc)
            p[key + "_buf"] = buf
    else:
        a = o["a"]
        if g["a_rows"] > M:        # rows behind M hold the sentinel: they are never read (and would show in the result)
            a = torch.cat([a, torch.full((g["a_rows"] - M, K), SENTINEL, dtype=BF)])
        p["a_buf"], p["a"] = R.strided(a, g["lda"], device, g["a_col"])
        p["w_buf"], p["w"] = R.strided(o["w"], g["ldw"], device)
    if case["out8"]:
        cbuf = torch.full((g["c_rows"], g["ldc"]), SENTINEL_U8, dtype=torch.uint8, device=device)
        p["bufs"]["C"] = cbuf
        p["bufs"]["Cs"] = torch.full((mx_scale_bytes(M, W),), SENTINEL_U8, dtype=torch.uint8, device=device)
        p["out"] = (cbuf[:, g["c_col"]:g["c_col"] + W], p["bufs"]["Cs"])
    else:
        cbuf = torch.full((g["c_rows"], g["ldc"]), SENTINEL, dtype=BF, device=device)
        p["bufs"]["C"] = cbuf
        p["out"] = cbuf[:, g["c_col"]:g["c_col"] + W]
    if "res" in o:
        if g["res_inplace"]:
            p["out"][:M].copy_(o["res"])
            p["kw"]["res"] = p["out"]
        else:
            p["res_buf"], p["kw"]["res"] = R.strided(o["res"], g["ldr"], device, g["r_col"])
    for key in ("bias", "scale", "out_rows"):
        if key in o:
            p["kw"][key] = o[key].to(device)
    if "row_scale" in o:
        keys = ("row_scale", "row_shift", "col_shift", "bias_f32") if "row_shift" in o else ("row_scale",)
        p["kw"]["folded_norm"] = tuple(o[k].to(device) for k in keys)
    if case["rowmap"] in ("group", "res_mod"):
        p["kw"].update(res_mod=PERIOD, res_off=1)
    if case["rowmap"] == "group":
        p["kw"].update(out_group=PERIOD, out_pad=1)
        if case["epi"] not in RESIDUAL:
            p["kw"].pop("res_mod"), p["kw"].pop("res_off")
    if g["a_rows"] > M:
        p["kw"]["M"] = M
    if case["rope_group"] is not None:
        if case["rope_place"] == "contig":
            qbuf = torch.full((M, g["ldq"]), SENTINEL, dtype=BF, device=device) if g["qw"] else None
            kbuf = torch.full((M, g["ldk"]), SENTINEL, dtype=BF, device=device)
            q, k = qbuf, kbuf
            if qbuf is not None:
                p["bufs"]["q"] = qbuf
            p["bufs"]["k"] = kbuf
        else:
            qk = torch.full((M, g["ldq"]), SENTINEL, dtype=BF, device=device)
            q = qk[:, g["q_col"]:g["q_col"] + g["qw"]] if g["qw"] else None
            k = qk[:, g["k_col"]:g["k_col"] + g["kw"]]
            p["bufs"]["qk"] = qk
        p["kw"]["rope"] = (o["cos"].to(device), o["sin"].to(device), o["pos"].to(device), q, k, case["rope_group"])
    return p


def views_of(p):
    """every placed 2-D view with its unit (2 = bf16 elements, 1 = bytes), for the alignment property"""
    out = []
    for key in ("a", "w", "out"):
        t = p[key]
        if isinstance(t, tuple):
            t = t[-2]
        out.append((key, t))
    if "res" in p["kw"]:
        out.append(("res", p["kw"]["res"]))
    if "rope" in p["kw"]:
        out += [(n, t) for n, t in (("rope_q", p["kw"]["rope"][3]), ("rope_k", p["kw"]["rope"][4])) if t is not None]
    return out


# ------------------------------------------------------------------------------------------------ expected images
def reference(case, o=None, device="cpu", vals=None):
    """the full expected image of every buffer the call may write (keys as place()'s ``bufs``), padding and unmapped rows
    included, plus ``written``: the cells of C the call stores (where SiLU-mul's tolerance applies).  ``device``: where the
    fp64 product is taken (the epilogue always runs on the CPU)."""
    o = operands(case) if o is None else o
    g = geometry(case)
    M, N, W = case["M"], case["N"], out_width(case)
    vals = values(case, o, device=device) if vals is None else vals
    img, c0 = {}, g["c_col"]
    if case["rope_group"] is not None:
        G = case["rope_group"]
        kv = N // ((G + 2) * 128)
        t = vals.view(M, kv, G + 2, 128)
        cs, sn = o["cos"][o["pos"].long()][:, None, None, :], o["sin"][o["pos"].long()][:, None, None, :]
        C = torch.full((M, g["ldc"]), SENTINEL, dtype=BF)
        written = torch.zeros(M, g["ldc"], dtype=torch.bool)
        for j in range(kv):                       # v heads in their own columns of C; every other column is left untouched
            lo = (j * (G + 2) + G + 1) * 128
            C[:, lo:lo + 128] = t[:, j, G + 1]
            written[:, lo:lo + 128] = True
        img["C"], img["written"] = C, written
        kr = R.rope_torch(t[:, :, G:G + 1], cs, sn).reshape(M, kv * 128)
        qr = R.rope_torch(t[:, :, :G], cs, sn).reshape(M, kv * G * 128) if G else None
        if case["rope_place"] == "contig":
            img["k"] = kr
            if G:
                img["q"] = qr
        else:
            qk = torch.full((M, g["ldq"]), SENTINEL, dtype=BF)
            qk[:, g["k_col"]:g["k_col"] + g["kw"]] = kr
            if G:
                qk[:, g["q_col"]:g["q_col"] + g["qw"]] = qr
            img["qk"] = qk
        return img
    rows = out_rows_of(case, o)
    written = torch.zeros(g["c_rows"], g["ldc"], dtype=torch.bool)
    written[rows, c0:c0 + W] = True
    if case["out8"]:
        codes, sb = mx_quantize(vals)
        C = torch.full((g["c_rows"], g["ldc"]), SENTINEL_U8, dtype=torch.uint8)
        C[rows, c0:c0 + W] = codes
        img["Cs"] = mx_scale_image(sb)
    else:
        C = torch.full((g["c_rows"], g["ldc"]), SENTINEL, dtype=BF)
        C[rows, c0:c0 + W] = vals
    img["C"], img["written"] = C, written
    return img


def compare(case, got, want):
    """the GPU test's comparison: every buffer equal to its expected image over its WHOLE extent - result cells, padding columns,
    unmapped rows, sentinels bit for bit - except the written cells of a SiLU-mul output, which keep test_gemm_silu_mul's bound.
    ``got``: buffers by name (any device).  Returns a list of failures (empty = pass)."""
    bad = []
    for name, ref in want.items():
        if name == "written":
            continue
        out = got[name].cpu()
        if out.shape != ref.shape or out.dtype != ref.dtype:
            bad.append(f"{name}: shape / dtype {tuple(out.shape)} {out.dtype} != {tuple(ref.shape)} {ref.dtype}")
            continue
        raw = lambda t: t.view(torch.int16) if t.dtype == BF else t
        if name == "C" and case["epi"] in ("silu", "rms_silu") and not case["out8"]:
            w = want["written"]
            if not torch.equal(raw(out)[~w], raw(ref)[~w]):
                bad.append(f"C: {int((raw(out)[~w] != raw(ref)[~w]).sum())} cells outside the output changed")
            a, b = out[w].float(), ref[w].float()
            u = R.ulps(out[w], ref[w])
            ok = (u <= SILU_BOUND["max_ulps"]) | ((a - b).abs() <= SILU_BOUND["atol"])
            if not bool(torch.isfinite(a).all()) or not bool(ok.all()):
                bad.append(f"C: {int((~ok).sum())} SiLU-mul cells beyond {SILU_BOUND['max_ulps']} ulps (max {int(u.max())})")
            elif float((u == 0).double().mean()) < SILU_BOUND["frac_exact"]:
                bad.append(f"C: only {float((u == 0).double().mean()):.4f} of the SiLU-mul cells bit-identical")
            continue
        # value equality on the cells the call writes (+0 == -0), bit equality everywhere else
        w = want["written"] if name == "C" and not case["out8"] else torch.zeros(ref.shape, dtype=torch.bool)
        if not torch.equal(raw(out)[~w], raw(ref)[~w]):
            n = int((raw(out)[~w] != raw(ref)[~w]).sum())
            bad.append(f"{name}: {n} cells the call must not write differ from their expected bits (padding, unmapped rows, sentinels)")
        if bool(w.any()) and not torch.equal(out[w], ref[w]):
            d = out[w] != ref[w]
            bad.append(f"{name}: {int(d.sum())} of {d.numel()} result cells differ")
    return bad


# ------------------------------------------------------------------------------------------------ addressing emulation
TILE_OF = {64: (64, 32), 128: (128, 128), 256: (256, 256), 2: (128, 256)}


def emulate(case, p, mutant=None, acc=None):
    """A kernel's ADDRESSING in torch, on flat storage: launch by launch, tile by tile, every cell is read from / written to
    base + row * ld + column, with the row maps taken from the absolute row (launch row + m_base) as gemm.hip does.  First the
    residual walk (what the launches READ), then the epilogue formula on it, then the store walk into the placed buffers ``p``
    (CPU).  ``mutant``: one of MUTANTS - the same walks with one subtle addressing mistake."""
    assert (mutant is None or mutant in MUTANTS) and not case["fp8"], mutant
    o, g = p["o"], p["g"]
    M, N, W = case["M"], case["N"], out_width(case)
    C = p["bufs"]["C"]
    flatC, ldc = C.view(-1), (W if mutant == "ldc_width" else C.stride(0))
    silu, rope = case["epi"] in ("silu", "rms_silu"), case["rope_group"] is not None

    def walk():
        for li, (row0, rows, fam) in enumerate(case["launches"]):
            bm, bn = TILE_OF[fam]
            bn = bn // 2 if silu else bn                     # (output columns of a tile)
            tiles_m, tiles_n = (rows + bm - 1) // bm, (W + bn - 1) // bn
            for tm in range(tiles_m):
                mrel = torch.arange(tm * bm, min(rows, (tm + 1) * bm))
                for tn in range(tiles_n):
                    final = li == len(case["launches"]) - 1 and tm == tiles_m - 1 and tn == tiles_n - 1
                    yield fam, row0, mrel, tn * bn, min(W, (tn + 1) * bn), final

    def put(flat, rows, ld, col0, src):
        idx = (rows[:, None] * ld + col0 + torch.arange(src.shape[1])[None, :]).reshape(-1)
        ok = idx < flat.numel()                              # (a store past the end of the buffer is dropped, not emulated)
        flat[idx[ok]] = src.reshape(-1)[ok]

    res = None
    if "res" in o:
        flatR = (C if g["res_inplace"] else p["res_buf"]).view(-1)
        ldr = N if mutant == "ldr_width" else p["kw"]["res"].stride(0)
        res = torch.zeros(M, N, dtype=BF)
        for fam, row0, mrel, n_lo, n_hi, _ in walk():
            mabs = row0 + mrel
            m_res = mrel if mutant == "res_mod_relative" else mabs
            rrow = 1 + m_res % PERIOD if case["rowmap"] in ("group", "res_mod") else mabs
            idx = rrow[:, None] * ldr + g["r_col"] + torch.arange(n_lo, n_hi)[None, :]
            res[mabs[:, None], torch.arange(n_lo, n_hi)[None, :]] = flatR[idx.clamp_max(flatR.numel() - 1)]
    vals = values(case, o, acc=acc, res=res)
    if rope:
        G = case["rope_group"]
        gs = (G + 2) * 128
        t = vals.view(M, N // gs, G + 2, 128)
        cs, sn = o["cos"][o["pos"].long()][:, None, None, :], o["sin"][o["pos"].long()][:, None, None, :]
        rot = R.rope_torch(t, cs, sn).reshape(M, N)          # (only the q / k slots of it are used)
        qt, kt = p["kw"]["rope"][3], p["kw"]["rope"][4]
        flatk = (p["bufs"]["k"] if "k" in p["bufs"] else p["bufs"]["qk"]).view(-1)
        if qt is not None:
            flatq = (p["bufs"]["q"] if "q" in p["bufs"] else p["bufs"]["qk"]).view(-1)
            ldq = g["qw"] if mutant == "ldq_width" else qt.stride(0)
    for fam, row0, mrel, n_lo, n_hi, final in walk():
        if mutant == "tile_unwritten" and final:
            continue
        mabs = row0 + mrel
        if rope:
            # a tile holds whole 128-wide heads (the fallback's narrower tiles: pieces of one): v to its columns of C, q / k rotated
            # to their de-interleaved buffers - the contract is the same whichever kernel runs the rows
            for lo in range(n_lo, n_hi, 128):
                hi = min(lo + 128, n_hi)
                head, d0 = lo - lo % 128, lo % 128
                grp = ((n_lo if fam == 256 and mutant == "kv_group_from_tile" else head)) // gs
                within = (head - grp * gs) >> 7
                if within == G + 1:
                    put(flatC, mabs, ldc, g["c_col"] + lo, vals[mabs, lo:hi])
                elif within == G:
                    put(flatk, mabs, kt.stride(0), g["k_col"] + grp * 128 + d0, rot[mabs, lo:hi])
                else:
                    put(flatq, mabs, ldq, g["q_col"] + (grp * G + within) * 128 + d0, rot[mabs, lo:hi])
            continue
        m_map = mrel if mutant == "out_group_relative" else mabs
        if case["rowmap"] == "rows" and mutant != "out_rows_ignored":
            orow = o["out_rows"][mabs].long()
        elif case["rowmap"] == "group":
            orow = (m_map // PERIOD) * (PERIOD + 1) + 1 + m_map % PERIOD
        else:
            orow = mabs
        cols = torch.arange(n_lo, n_hi + (8 if mutant == "cols_past_n" and n_hi == W else 0))
        put(flatC, orow, ldc, g["c_col"] + n_lo, vals[mabs][:, cols.clamp_max(W - 1)])
    return p["bufs"]


def mutant_applies(case, mutant):
    """the cases on which a mutant's mistake changes an address"""
    if case["fp8"] or case["refuse"]:
        return False
    g = geometry(case)
    rope, W = case["rope_group"] is not None, out_width(case)
    apart = case["epi"] in RESIDUAL and not g["res_inplace"]
    peeled = len(case["launches"]) == 2
    fused = case["launches"][0][2] == 256 and not peeled
    return {
        "ldc_width": g["ldc"] != W,
        "ldr_width": case["epi"] in RESIDUAL and g["ldr"] != case["N"],
        "res_mod_relative": case["rowmap"] == "group" and apart and peeled,
        "out_group_relative": case["rowmap"] == "group" and peeled,
        "out_rows_ignored": case["rowmap"] == "rows",
        "tile_unwritten": True,
        "cols_past_n": not rope and g["ldc"] - g["c_col"] - W >= 8,
        "kv_group_from_tile": rope and case["rope_group"] == 1 and fused,
        "ldq_width": rope and case["rope_group"] > 0 and case["rope_place"] == "slices",
    }[mutant]
