"""GEMM addressing on the MI355X: every case of gemm_ref.cases() - kernel form x operand layout x epilogue, the row maps, the rotary
groups - is ONE ops.gemm call on operands placed in sentinel-filled buffers, and every buffer the call may write must equal its
expected image over its whole extent: result cells (bit-exact by construction; SiLU-mul within test_gemm_silu_mul's bound), padding
columns, unmapped rows and sentinels bit for bit.  Before the launch the plan must be the form the case is named for.  What the
comparison catches is shown on the CPU (test_gemm_refs.py).

Rotary cases on rows that take the fallback (tile 64 / 128, a peeled tail): include/mjv.h's "the other columns of C are left
untouched" is what the expected image holds.  The fallback used to write the whole un-rotated Linear into C (its launch was a plain
EPI_BIAS one); it now stores the q / k heads in rope_q / rope_k and rotates them there."""
import pytest
import torch

import gemm_ref as G

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


@pytest.fixture(scope="module")
def device_cases(cuda):
    c = torch.cuda.get_device_properties(cuda).multi_processor_count
    return c, {case["name"]: case for case in G.cases(c)}


@pytest.fixture(scope="module")
def workspace(cuda):
    from mj_video_amd import ops
    return torch.empty(ops.gemm_workspace_bytes(), dtype=torch.uint8, device=cuda)


def call_of(case, p, workspace):
    """(a, w, out, keywords) of the ops.gemm call of a placed case"""
    from mj_video_amd import ops
    code = dict(bias=ops.EPI_BIAS, nobias=ops.EPI_BIAS, ln_bias=ops.EPI_BIAS, gelu=ops.EPI_BIAS_GELU, ln_gelu=ops.EPI_BIAS_GELU,
                relu=ops.EPI_BIAS_RELU, scale_res=ops.EPI_SCALE_RES, res=ops.EPI_SCALE_RES, silu=ops.EPI_SILU_MUL,
                rms_silu=ops.EPI_SILU_MUL, rope=ops.EPI_ROPE_QKV)[case["epi"]]
    kw = dict(p["kw"], epilogue=code, tile=case["tile"])
    if case["ws"]:
        kw["workspace"] = workspace
    a, w, out = p["a"], p["w"], p["out"]
    if case["fp8"]:
        a, w = (ops.quantize_mxfp8(vals, out=ops.MX8(view, scales)) for vals, view, scales in (a, w))
        if case["out8"]:
            out = ops.MX8(*out)
    return a, w, out, kw


def launches_recorded(fn):
    from mj_video_amd import ops
    ops.prof_filter(None)
    ops.prof_reset()
    ops.prof_enable(True)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        ops.prof_enable(False)
    tags = ops.prof_results()
    ops.prof_reset()
    return tags


@pytest.mark.parametrize("name", [case["name"] for case in G.cases(256)])
def test_gemm_layout(cuda, device_cases, workspace, name):
    from mj_video_amd import ops, _lib
    c, table = device_cases
    case = table[name]
    p = G.place(case, cuda)
    a, w, out, kw = call_of(case, p, workspace)
    if case["refuse"]:
        # tile 2 and MXFP8 operands write plain rows only: every row map is refused before anything is launched
        before = {k: v.clone() for k, v in p["bufs"].items()}

        def refused():
            with pytest.raises((_lib.MjvLibraryError, AssertionError)):
                ops.gemm(a, w, out, **kw)

        assert launches_recorded(refused) == {}
        assert all(torch.equal(before[k], p["bufs"][k]) for k in before)
        return
    plan = ops.gemm_plan(a, w, out, **kw)
    got = [(L["family"], L["split"] > 1, L["persistent"], L["rope_split_after"]) for L in plan["launches"]]
    assert got == case["plan"] or 0 <= c < case["min_cus"] or (case["min_cus"] < 0 and c != -case["min_cus"]), (c, plan)
    if case["fp8"]:       # the quantiser stayed inside its views, and the operands are what the reference multiplies
        for key in ("a", "w"):
            col = p["g"]["a_col"] if key == "a" else 0
            assert G.R.padding_untouched(p[key + "_buf"], col, case["K"], G.SENTINEL_U8)
    ops.gemm(a, w, out, **kw)
    torch.cuda.synchronize()
    want = G.reference(case, p["o"], device=cuda)
    bad = G.compare(case, p["bufs"], want)
    assert not bad, (name, plan, bad)
    # the operands are read-only: their buffers, padding included, are as placed
    if not case["fp8"]:
        fresh = G.place(case, "cpu", p["o"])
        assert torch.equal(p["a_buf"].cpu(), fresh["a_buf"]) and torch.equal(p["w_buf"].cpu(), fresh["w_buf"])
        if "res_buf" in p:
            assert torch.equal(p["res_buf"].cpu(), fresh["res_buf"])
