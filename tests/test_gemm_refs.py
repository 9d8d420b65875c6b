"""The claims of gemm_ref.py, proven on the CPU: the operands make every case exact, the case table covers every (form, epilogue),
(form, layout) and (form, row map) pair, every placed view is inside the header's alignment contract, every case takes the kernel
form it is named for (mjv_gemm_plan needs no GPU), and the comparison of test_gemm_layouts_gpu.py fails on each of nine subtle
addressing mistakes.  No GPU is touched."""
import ctypes as C
import os

import pytest
import torch

import gemm_ref as G
from rowops_ref import BF

CUS = (256, 64)
CASES = {c: G.cases(c) for c in CUS}
UNIQUE = {(case["name"], case["M"]): case for c in CUS for case in CASES[c]}      # (most shapes do not depend on the CU count)
SMALL = [case for case in CASES[64] if not case["fp8"] and not case["refuse"]]
EPI_CODE = dict(bias=0, nobias=0, ln_bias=0, gelu=1, ln_gelu=1, relu=2, scale_res=3, res=3, silu=4, rms_silu=4, rope=5)


@pytest.mark.parametrize("key", list(UNIQUE), ids=lambda k: f"{k[0]}-M{k[1]}")
def test_every_case_is_exact(key):
    """the precondition (every partial sum below 2^24 quanta), and its consequence: fp32 arithmetic with K summed in 64-wide
    chunks in reversed order gives the fp64 reference's bits.  SiLU-mul cases: up to the bf16 gate / up values, the last exact
    point before the one transcendental.  MXFP8 cases: the block quantiser represents the operands exactly."""
    case = UNIQUE[key]
    o = G.operands(case)
    assert G.max_partial_sum(case, o) < 2 ** 24
    if case["fp8"]:
        for t in (o["a"], o["w"]):
            assert torch.equal(G.mx_dequantize(*G.mx_quantize(t)), t.float())
    if case["refuse"]:
        return
    probe = dict(case, epi="nobias") if case["epi"] in ("silu", "rms_silu") else case
    v64 = G.values(probe, o)
    v32 = G.values(probe, o, dtype=torch.float32, chunked=True)
    assert v64.dtype == BF and torch.equal(v64.view(torch.int16), v32.view(torch.int16))


def test_silu_share_of_an_fp32_formula():
    """SiLU-mul is the one non-exact epilogue: what an fp32 x * rcp(1 + e^-x) reaches against the fp64 reference on these very
    inputs is inside the bound the GPU test keeps (test_gemm_silu_mul's), with room"""
    worst_share, beyond = 1.0, 0
    for case in UNIQUE.values():
        if case["epi"] in ("silu", "rms_silu") and not case["refuse"]:
            share, u = G.silu_fp32_share(case, G.operands(case))
            worst_share, beyond = min(worst_share, share), beyond + u
    print(f"fp32 SiLU-mul against fp64: at least {worst_share:.5f} of a case's cells bit-identical, {beyond} cells beyond 3 ulps / 2e-3")
    assert worst_share >= G.SILU_BOUND["frac_exact"] and beyond == 0


@pytest.mark.parametrize("cus", CUS)
def test_the_table_covers_every_pair(cus):
    live = [c for c in CASES[cus] if not c["refuse"] and c["rope_group"] is None]
    have_epi = {(c["form"], c["epi"] + ("_out8" if c["out8"] else "")) for c in live}
    have_layout = {(c["form"], c["layout"]) for c in live}
    have_map = {(c["form"], c["rowmap"]) for c in live}
    for form in G.form_names():
        epis, layouts, maps = G.form_accepts(form)
        assert not [e for e in epis if (form, e) not in have_epi], form
        assert not [x for x in layouts if (form, x) not in have_layout], form
        assert not [m for m in maps if (form, m) not in have_map], form
    # the out_rows fallback of the K-sliced / peeled shapes, the refusals, the rotary matrix
    for form in ("t256_sliced", "peeled_128_tail", "peeled_skinny_tail"):
        assert (form, "rows") in have_map
    refused = {(c["form"], c["rowmap"]) for c in CASES[cus] if c["refuse"]}
    assert refused == {(f, m) for f in ("two_per_cu", "f8_t256") for m in ("group", "rows", "res_mod")}
    rope = {(c["form"], c["rope_group"], c["rope_place"]) for c in CASES[cus] if c["rope_group"] is not None}
    assert {(g, p) for f, g, p in rope if f == "t256"} == {(g, p) for g in (0, 1, 2, 4) for p in ("contig", "slices")}
    for form in ("t128", "skinny64"):
        assert {g for f, g, _ in rope if f == form} == {0, 1, 2, 4}
    assert ("peeled_128_tail", 2, "slices") in rope
    assert len({c["name"] for c in CASES[cus]}) == len(CASES[cus])


def test_every_placed_view_is_inside_the_alignment_contract():
    """include/mjv.h: leading dimensions multiples of 8 elements (MXFP8: 16 bytes), 16-byte aligned base pointers"""
    for case in CASES[64]:
        if case["refuse"]:
            continue
        p = G.place(case)
        for name, t in G.views_of(p):
            unit = t.element_size()
            assert t.stride(1) == 1 and t.data_ptr() % 16 == 0, (case["name"], name)
            if name == "out" and case["out8"]:
                assert (t.stride(0) * unit) % 8 == 0, (case["name"], name)     # (an MX8 output row is stored in 8-byte pieces)
            else:
                assert (t.stride(0) * unit) % 16 == 0, (case["name"], name, t.stride(0))
        for t in p["kw"].get("folded_norm", ()):
            assert t.data_ptr() % 16 == 0 and t.numel() % 256 == 0
        for key in ("bias", "scale"):
            assert key not in p["kw"] or p["kw"][key].data_ptr() % 16 == 0


# ------------------------------------------------------------------------------------------------ the plan, without a GPU
@pytest.fixture(scope="module")
def lib():
    from mj_video_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        _lib.build_library()
    return _lib.load_library()


def desc_of(lib, case):
    """the descriptor ops.gemm would fill for a placed case, with dummy pointers at the case's column offsets (planning
    dereferences nothing; tests/test_gemm_plan_host.py)"""
    from mj_video_amd import _lib
    PTR = 0x100000
    g = G.geometry(case)
    unit = 1 if case["fp8"] else 2
    d = _lib.GemmDesc()
    d.A, d.lda, d.W, d.ldw = PTR + g["a_col"] * unit, g["lda"], PTR, g["ldw"]
    d.C, d.ldc = PTR + g["c_col"] * (1 if case["out8"] else 2), g["ldc"]
    d.M, d.N, d.K, d.epilogue, d.tile = case["M"], case["N"], case["K"], EPI_CODE[case["epi"]], case["tile"]
    if case["epi"] in G.RESIDUAL:
        d.res, d.ldr = PTR + g["r_col"] * 2, g["ldr"]
    if case["epi"] in ("bias", "gelu", "relu", "scale_res"):
        d.bias = PTR
    if case["rowmap"] in ("group", "res_mod") and case["epi"] in G.RESIDUAL:
        d.res_mod, d.res_off = G.PERIOD, 1
    if case["rowmap"] == "group":
        d.out_group, d.out_pad = G.PERIOD, 1
    if case["rowmap"] == "rows":
        d.out_rows = PTR
    if case["rope_group"] is not None:
        d.rope_cos = d.rope_sin = d.rope_pos = PTR
        d.rope_q, d.rope_k = (PTR + g["q_col"] * 2 if g["qw"] else None), PTR + g["k_col"] * 2
        d.rope_ldq, d.rope_ldk, d.rope_group = g["ldq"], g["ldk"], case["rope_group"]
    if case["fp8"]:
        d.a_format = d.w_format = _lib.FMT_MXFP8
        d.a_scales = d.w_scales = PTR
        if case["out8"]:
            d.c_format, d.c_scales = _lib.FMT_MXFP8, PTR
    if case["epi"] in ("ln_bias", "ln_gelu", "rms_silu"):
        d.row_scale = PTR
        if case["epi"] != "rms_silu":
            d.row_shift = d.col_shift = d.bias_f32 = PTR
    if case["ws"]:
        d.workspace, d.workspace_bytes = PTR, lib.mjv_gemm_workspace_bytes()
    return d


@pytest.mark.parametrize("cus", CUS)
def test_every_case_takes_the_form_it_is_named_for(lib, cus):
    from mj_video_amd import ops
    for case in CASES[cus]:
        d = desc_of(lib, case)
        if case["refuse"]:
            assert lib.mjv_gemm_plan(C.byref(d), cus, None, 0) < 0, case["name"]
            continue
        plan = ops.gemm_desc_plan(d, cus)
        got = [(L["family"], L["split"] > 1, L["persistent"], L["rope_split_after"]) for L in plan["launches"]]
        if case["min_cus"] >= 0 and cus >= case["min_cus"] or cus == -case["min_cus"]:
            assert got == case["plan"], (case["name"], cus, plan)
            assert [(L["row0"], L["rows"], L["family"]) for L in plan["launches"]] == case["launches"], (case["name"], plan)


# ------------------------------------------------------------------------------------------------ the comparison can fail
def run_emulation(case, mutant=None):
    p = G.place(case)
    return G.compare(case, G.emulate(case, p, mutant), G.reference(case, p["o"]))


@pytest.mark.parametrize("case", SMALL, ids=lambda c: c["name"])
def test_a_correct_walk_passes_the_comparison(case):
    assert run_emulation(case) == []


@pytest.mark.parametrize("mutant", G.MUTANTS)
def test_every_mutant_is_caught(mutant):
    """ld = width on C / on res, the launch-relative row in res_mod / out_group, out_rows ignored, one tile left unwritten, 8 columns
    written past N, the kv group taken from the tile instead of the head, q written at ldq = width: each fails the comparison on
    EVERY case where it changes an address, and there are such cases"""
    hit = [case for case in SMALL if G.mutant_applies(case, mutant)]
    assert hit, mutant
    missed = [case["name"] for case in hit if not run_emulation(case, mutant)]
    assert not missed, (mutant, missed)
