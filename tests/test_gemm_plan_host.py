"""The GEMM launch plan (csrc/gemm_plan.h, exported as mjv_gemm_plan) read without a GPU: the launches KERNELS.md documents for
the model's shapes on 256 compute units, the refusals, and the contracts of include/mjv.h / DESIGN §9 over a grid of shapes,
epilogues, both operand formats and partition sizes (32 - 256 CUs).  Pointers are dummies: planning dereferences nothing."""
import ctypes as C
import itertools
import os

import pytest

from mj_video_amd import _lib, ops

BIAS, GELU, RELU, SCALE_RES, SILU_MUL, ROPE_QKV = range(6)
PTR = 0x10000    # non-null, 16-byte aligned, never dereferenced
KEYS = ("family", "epilogue", "row0", "rows", "split", "persistent", "rope_split_after")
T2_MESSAGE = ("gemm: tile 2 (128 x 256, two workgroups per CU) takes bias / bias + GELU / LayerScale + residual epilogues on plain, "
              "16-byte aligned output rows")
FOLD_MESSAGE = ("gemm: the 256-tile kernel has no instantiation for epilogue {} with {} folded in (bias / bias+GELU take a "
                "LayerNorm: row_scale + row_shift; SiLU-mul / RoPE-qkv an RMSNorm: row_scale only)")


@pytest.fixture(scope="module")
def lib():
    if not os.path.isfile(_lib.LIB_PATH):
        _lib.build_library()
    return _lib.load_library()


def desc(lib, M, N, K, epi, fp8=False, out8=False, ws=True, tile=0, rope_group=2, fold=0):
    """fold: 1 = an RMSNorm (row_scale), 2 = a LayerNorm (row_scale, row_shift, col_shift, bias_f32) folded in; ws: True = a
    workspace of mjv_gemm_workspace_bytes(), an int = that many bytes, False = none"""
    d = _lib.GemmDesc()
    d.A = d.W = d.C = PTR
    d.lda = d.ldw = K
    d.M, d.N, d.K, d.epilogue, d.tile = M, N, K, epi, tile
    d.ldc = N // 2 if epi == SILU_MUL else N
    if epi == SCALE_RES:
        d.res, d.ldr = PTR, N
    if epi == ROPE_QKV:
        d.rope_cos = d.rope_sin = d.rope_pos = d.rope_q = d.rope_k = PTR
        d.rope_ldq, d.rope_ldk, d.rope_group = N, N, rope_group
    if fp8:
        d.a_format = d.w_format = _lib.FMT_MXFP8
        d.a_scales = d.w_scales = PTR
        if out8:
            d.c_format, d.c_scales = _lib.FMT_MXFP8, PTR
    if fold:
        d.row_scale = PTR
        if fold == 2:
            d.row_shift = d.col_shift = d.bias_f32 = PTR
    if ws:
        d.workspace, d.workspace_bytes = PTR, (lib.mjv_gemm_workspace_bytes() if ws is True else ws)
    return d


def launches(lib, *args, cus=256, **kw):
    return [tuple(L[k] for k in KEYS) for L in ops.gemm_desc_plan(desc(lib, *args, **kw), cus)["launches"]]


def refusal(lib, d, cus=256):
    rc = lib.mjv_gemm_plan(C.byref(d), cus, None, 0)
    return int(rc), lib.mjv_last_error().decode()


# (M, N, K, epilogue, MXFP8 operands) -> launches (family, epilogue, row0, rows, split, persistent, rope_split_after) on 256 CUs, each
# derived by hand from the rules of gemm_plan.h; KERNELS.md / DESIGN §9 state them as facts
DOCUMENTED = [
    # ViT proj / fc2: 257 x 4 = 1028 tiles = 4 rounds + 4 -> the 64 CLS-ragged rows go to the skinny kernel
    ((65600, 1024, 1024, SCALE_RES, False), [(256, SCALE_RES, 0, 65536, 1, 0, 0), (64, SCALE_RES, 65536, 64, 1, 0, 0)]),
    # ViT qkv: 3084 tiles = 12 rounds + 12; plain bias with 16 K-tiles -> the persistent form
    ((65600, 3072, 1024, BIAS, False), [(256, BIAS, 0, 65536, 1, 1, 0), (64, BIAS, 65536, 64, 1, 0, 0)]),
    # ViT fc1: 4112 tiles = 16 rounds + 16; the GELU epilogue keeps the one-tile kernel
    ((65600, 4096, 1024, GELU, False), [(256, GELU, 0, 65536, 1, 0, 0), (64, GELU, 65536, 64, 1, 0, 0)]),
    # w1|w3: 4288 tiles = 16 rounds + 192 (a last round that is 3/4 full stays)
    ((16976, 16384, 2048, SILU_MUL, False), [(256, SILU_MUL, 0, 16976, 1, 1, 0)]),
    # w2: 536 tiles = 2 rounds + 24 -> 592 rows (3 x 8 tiles) K-sliced: min(256 / 24, split_max 8, 128 / 8)
    ((16976, 2048, 8192, SCALE_RES, False), [(256, SCALE_RES, 0, 16384, 1, 0, 0), (256, SCALE_RES, 16384, 592, 8, 0, 0)]),
    # wo: the same rows at K = 2048 (32 K-tiles: too shallow for either slicing)
    ((16976, 2048, 2048, SCALE_RES, False), [(256, SCALE_RES, 0, 16384, 1, 0, 0), (128, SCALE_RES, 16384, 592, 1, 0, 0)]),
    # wqkv: 1072 tiles = 4 rounds + 48; the tail has no rotary epilogue: plain Linear, then rope_split
    ((16976, 4096, 2048, ROPE_QKV, False), [(256, ROPE_QKV, 0, 16384, 1, 0, 0), (128, BIAS, 16384, 592, 1, 0, 1)]),
    # MXFP8 fc2: the 64-row tail is 4 tiles: min(256 / 4, 32 K-tiles / 2, 32) slices
    ((65600, 1024, 4096, SCALE_RES, True), [(256, SCALE_RES, 0, 65536, 1, 0, 0), (256, SCALE_RES, 65536, 64, 16, 0, 0)]),
    # MXFP8 w2: 24 tiles: min(256 / 24, 64 / 2, 32)
    ((16976, 2048, 8192, SCALE_RES, True), [(256, SCALE_RES, 0, 16384, 1, 0, 0), (256, SCALE_RES, 16384, 592, 10, 0, 0)]),
    # 3 x 4 tiles of 128: min(512 / 12, split_max 8, 64 / 4); the 256-tile slicing refuses a last m-tile under 70 % full (44 of 256)
    ((300, 512, 4096, BIAS, False), [(128, BIAS, 0, 300, 8, 0, 0)]),
]
IDS = ["{}x{}x{}-epi{}{}".format(*p[:4], "-mxfp8" if p[4] else "") for p, _ in DOCUMENTED]


@pytest.mark.parametrize("problem,want", DOCUMENTED, ids=IDS)
def test_documented_launches_on_256_cus(lib, problem, want):
    M, N, K, epi, fp8 = problem
    plan = ops.gemm_desc_plan(desc(lib, M, N, K, epi, fp8=fp8), 256)
    assert [tuple(L[k] for k in KEYS) for L in plan["launches"]] == want
    for L in plan["launches"]:
        assert L["grid"] == 256 if L["persistent"] else L["grid"] > 0


@pytest.mark.parametrize("problem,want", DOCUMENTED, ids=IDS)
def test_documented_problems_without_workspace_and_with_a_forced_tile(lib, problem, want):
    M, N, K, epi, fp8 = problem
    bare = launches(lib, M, N, K, epi, fp8=fp8, ws=False)
    assert all(L[4] == 1 for L in bare), "no K slices without a workspace"
    if fp8:
        assert len(bare) == 1, "an MXFP8 tail only ever runs sliced: no workspace, no peel"
    else:
        assert [L[2:4] for L in bare] == [L[2:4] for L in want], "bf16 tails are peeled all the same (128-tiles, unsliced)"
        assert [L for L in bare if L[4] == 1 and L in want] == [L for L in want if L[4] == 1], "unsliced launches stay as they are"
    for tile in (64, 128, 256):
        forced = launches(lib, M, N, K, epi, fp8=fp8, tile=tile)
        # (one tile kernel exists for MXFP8 operands: every forced tile is the one unsliced 256-tile launch)
        assert len(forced) == 1 and forced[0][0] == (256 if fp8 else tile) and forced[0][2:4] == (0, M)
        if fp8:
            assert forced[0][4] == 1


def test_tile_code_2_inside_and_outside_its_domain(lib):
    for epi in (BIAS, GELU, SCALE_RES):
        assert launches(lib, 65600, 1024, 1024, epi, tile=2) == [(2, epi, 0, 65600, 1, 0, 0)]
    outside = [desc(lib, 1000, 512, 256, epi, tile=2) for epi in (RELU, SILU_MUL, ROPE_QKV)] + [desc(lib, 1000, 512, 256, BIAS, tile=2, fold=1)]
    rows = desc(lib, 1000, 512, 256, BIAS, tile=2)
    rows.out_rows = PTR
    grouped = desc(lib, 1000, 512, 256, BIAS, tile=2)
    grouped.out_group = 100
    for d in outside + [rows, grouped]:
        assert refusal(lib, d) == (-3, T2_MESSAGE)
    # (an output that is not 16-byte aligned no longer reaches the tile-2 rule: the descriptor check refuses it for every family)
    odd_c = desc(lib, 1000, 512, 256, BIAS, tile=2)
    odd_c.C = PTR + 8
    assert refusal(lib, odd_c) == (-1, "gemm: misaligned pointer")


@pytest.mark.parametrize("epi", [BIAS, GELU, RELU, SILU_MUL, ROPE_QKV])
@pytest.mark.parametrize("fold", [1, 2])
def test_folded_norm_instantiation_table(lib, epi, fold):
    """the unsliced 256-tile kernels instantiate a LayerNorm (2) for BIAS / BIAS_GELU and an RMSNorm (1) for SILU_MUL / ROPE_QKV;
    the small kernels and the K-sliced finish take every pair (SCALE_RES takes none: an argument error)"""
    in_table = {BIAS: 2, GELU: 2, SILU_MUL: 1, ROPE_QKV: 1}.get(epi) == fold
    for M, K in ((1024, 256), (65600, 1024)):        # one launch; a peeled one (refused as a whole: nothing runs)
        d = desc(lib, M, 1024, K, epi, fold=fold)
        if in_table:
            assert all(L["family"] in (256, 64) for L in ops.gemm_desc_plan(d, 256)["launches"])
        else:
            assert refusal(lib, d) == (-3, FOLD_MESSAGE.format(epi, "row_scale + row_shift" if fold == 2 else "row_scale"))
    assert [L[0] for L in launches(lib, 300, 1024, 256, epi, fold=fold)] == [128]
    assert [L[0] for L in launches(lib, 64, 1024, 256, epi, fold=fold)] == [64]
    sliced = launches(lib, 592, 2048, 8192, epi, fold=fold)
    assert [(L[0], L[4]) for L in sliced] == [(256, 8)]
    rc, msg = refusal(lib, desc(lib, 1024, 1024, 256, SCALE_RES, fold=fold))
    assert rc == -1 and msg == "gemm: no norm is folded into the residual epilogue"


@pytest.mark.parametrize("M", [1, 64, 128])
def test_up_to_128_rows_are_one_skinny_launch(lib, M):
    for N, K, epi, cus in itertools.product((256, 16384), (128, 8192), (BIAS, SCALE_RES, SILU_MUL, ROPE_QKV), (32, 256)):
        rope = epi == ROPE_QKV
        assert launches(lib, M, N, K, epi, cus=cus, rope_group=0) == [(64, BIAS if rope else epi, 0, M, 1, 0, int(rope))]


def test_the_plan_call_checks_like_the_gemm_call_and_respects_the_buffer(lib):
    d = desc(lib, 16976, 2048, 8192, SCALE_RES)
    n = lib.mjv_gemm_plan(C.byref(d), 256, None, 0)
    assert n == 4 + 8 * 2
    buf = (C.c_int32 * (n + 8))(*([-7] * (n + 8)))
    assert lib.mjv_gemm_plan(C.byref(d), 256, buf, n) == n
    assert list(buf[n:]) == [-7] * 8 and list(buf[:4]) == [2, 4, 1, 0]     # K = 8192: group-M 4; 69.5 MB out: streaming stores
    again = (C.c_int32 * n)()
    assert lib.mjv_gemm_plan(C.byref(d), 256, again, n) == n and list(again) == list(buf[:n])
    short = (C.c_int32 * n)(*([-7] * n))
    assert lib.mjv_gemm_plan(C.byref(d), 256, short, n - 1) == -1 and b"gemm_plan" in lib.mjv_last_error()
    assert list(short) == [-7] * n
    # the descriptor checks are those of mjv_gemm_bf16, message for message
    for change, text in ((dict(K=100), "gemm: K=100 must be a multiple of 64"), (dict(tile=100), "gemm: tile 100 not in {0, 2, 64, 128, 256}"),
                         (dict(epilogue=6), "gemm: unknown epilogue 6"), (dict(A=0), "gemm: null pointer")):
        bad = desc(lib, 512, 512, 256, BIAS)
        if "K" in change:
            bad.lda = bad.ldw = 104
        for k, v in change.items():
            setattr(bad, k, v)
        assert refusal(lib, bad) == (-1, text)
        assert lib.mjv_gemm_bf16(C.byref(bad), None) == -1 and lib.mjv_last_error().decode() == text
    bad = desc(lib, 512, 512, 256, ROPE_QKV, fp8=True)
    assert refusal(lib, bad) == (-1, "gemm(mxfp8): epilogue 5 unsupported")


@pytest.mark.parametrize("family", [0, 64, 128, 256, 2, "mxfp8"])
def test_the_header_alignment_contract_is_enforced_for_every_family(lib, family):
    """include/mjv.h: ldc / ldr % 8, C and res 16-byte aligned, bias / scale 8-byte aligned - whichever kernel the plan would pick
    (the 256-tile, persistent, tile-2 and rotary paths move 16-byte pieces of those rows).  Each violation is an argument error of
    the plan query and of the GEMM call itself, before anything is launched (no GPU is needed to be refused)."""
    fp8 = family == "mxfp8"
    pre = "gemm(mxfp8): " if fp8 else "gemm: "
    res_text = pre + "the residual needs ldr % 8 == 0 and a 16-byte aligned pointer"
    c_text = pre + ("ldc / C alignment" if fp8 else "misaligned pointer")
    violations = [(dict(ldc=1024 + 4), pre + ("ldc / C alignment" if fp8 else "leading dims must be multiples of 8")),
                  (dict(C=PTR + 8), c_text), (dict(C=PTR + 4), c_text), (dict(ldr=1024 + 4), res_text), (dict(res=PTR + 8), res_text),
                  (dict(bias=PTR + 4), pre + "bias / scale must be 8-byte aligned"), (dict(scale=PTR + 2), pre + "bias / scale must be 8-byte aligned")]
    for M in (64, 1000, 65600):
        good = desc(lib, M, 1024, 1024, SCALE_RES, fp8=fp8, tile=0 if fp8 else family)
        good.bias = good.scale = PTR + 8
        assert lib.mjv_gemm_plan(C.byref(good), 256, None, 0) > 0, lib.mjv_last_error()
        for change, text in violations:
            bad = desc(lib, M, 1024, 1024, SCALE_RES, fp8=fp8, tile=0 if fp8 else family)
            bad.bias = bad.scale = PTR + 8
            for k, v in change.items():
                setattr(bad, k, v)
            assert refusal(lib, bad) == (-1, text), (M, change)
            assert lib.mjv_gemm_bf16(C.byref(bad), None) == -1 and lib.mjv_last_error().decode() == text, (M, change)
    # a residual that no epilogue reads is not checked; an MX8 output keeps its own 8-byte rule
    free = desc(lib, 1000, 1024, 1024, BIAS, fp8=fp8, tile=0 if fp8 else family)
    free.res, free.ldr = PTR + 2, 1023
    assert lib.mjv_gemm_plan(C.byref(free), 256, None, 0) > 0


# ------------------------------------------------------------------------------------------- contracts over a grid
MS = (1, 64, 128, 129, 511, 512, 592, 2186, 16976, 17488, 65600)
NS = (256, 1024, 2048, 4096, 16384)
KS = (128, 1024, 2048, 8192)
SLICE_BYTES = {128: 65536, 256: 262144}     # fp32 accumulators of one K slice of one tile


def check_contracts(lib, M, N, K, epi, fp8, out8, ws, cus):
    d = desc(lib, M, N, K, epi, fp8=fp8, out8=out8, ws=ws, rope_group=2 if N % 512 == 0 else 0)
    plan = ops.gemm_desc_plan(d, cus)
    ls = plan["launches"]
    what = (M, N, K, epi, fp8, out8, ws, cus, ls)
    assert 1 <= len(ls) <= 2, what
    # the row ranges partition [0, M) in order; a peeled main launch is whole 256-row tiles (and whole 64-row scale groups)
    assert ls[0]["row0"] == 0 and all(L["rows"] > 0 for L in ls) and sum(L["rows"] for L in ls) == M, what
    if len(ls) == 2:
        assert ls[1]["row0"] == ls[0]["rows"] and ls[0]["rows"] % 256 == 0, what
    for L in ls:
        fam = L["family"]
        assert fam in ((256,) if fp8 else (64, 128, 256)), what
        bm, bn = (64, 32) if fam == 64 else (fam, fam)
        tiles = -(-L["rows"] // bm) * -(-N // bn)
        assert L["split"] >= 1, what
        if L["split"] > 1:
            assert ws and fam in SLICE_BYTES and L["split"] * tiles * SLICE_BYTES[fam] <= d.workspace_bytes, what
        if L["persistent"]:
            nk = K // 64
            assert not fp8 and fam == 256 and L["split"] == 1 and L["epilogue"] in (BIAS, RELU, SILU_MUL), what
            assert tiles > cus and nk >= 4 and nk % 2 == 0 and L["grid"] == cus, what
        else:
            assert L["grid"] == tiles * L["split"], what
        fallback = epi == ROPE_QKV and not (fam == 256 and L["split"] == 1)
        assert L["rope_split_after"] == int(fallback) and L["epilogue"] == (BIAS if fallback else epi), what
    assert ops.gemm_desc_plan(d, cus) == plan, "deterministic"
    return plan


@pytest.mark.parametrize("cus", [32, 64, 128, 256])
@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "mxfp8"])
def test_contracts_hold_over_shapes_epilogues_workspaces(lib, fp8, cus):
    """include/mjv.h (mjv_gemm_plan, mjv_gemm_desc.workspace / tile) and DESIGN §9 - not a second copy of the planner: row
    coverage, whole-tile main launches, slices only through a workspace that holds them, the persistent form's domain, the
    rotary fallback.  A 1 MiB workspace (4 slices of one 256-tile) is walked beside the full-size one and none."""
    seen = set()
    for M, N, K, ws in itertools.product(MS, NS, KS, (True, 1 << 20, False)):
        if fp8:
            cases = [(e, o) for e in (BIAS, GELU, RELU, SCALE_RES, SILU_MUL) for o in (False, True) if not (o and e == SCALE_RES)]
        else:
            cases = [(e, False) for e in (BIAS, GELU, RELU, SCALE_RES, SILU_MUL, ROPE_QKV)]
        for epi, out8 in cases:
            plan = check_contracts(lib, M, N, K, epi, fp8, out8, ws, cus)
            seen |= {(len(plan["launches"]), L["family"], L["split"] > 1, L["persistent"], L["rope_split_after"]) for L in plan["launches"]}
    # the walk reached every branch it is meant to judge
    assert {s[0] for s in seen} == {1, 2} and any(s[2] for s in seen)
    if not fp8:
        assert {s[1] for s in seen} == {64, 128, 256} and any(s[3] for s in seen) and any(s[4] for s in seen)
        assert any(s[1] == 128 and s[2] for s in seen) and any(s[1] == 256 and s[2] for s in seen)
