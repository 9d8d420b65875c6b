"""Reference and bound of the attention readout (test infrastructure only; shared by the kernel and the model tests of
tests/test_readout_gpu.py): the float64 softmax of the SAME bf16 queries and keys, binned as the plan says, and the bound of
include/mjv.h's definition worked out from those inputs - never from what the kernel returns."""
import numpy as np
import torch


def gather_keys(tensors, ranges, kv_heads, D, khs):
    """the key rows of one query, [L, kv_heads, D] float64 (``tensors``: host bf16 tensors, first kv head at column 0)"""
    parts = []
    for t, r0, n in ranges:
        rows = tensors[t][r0:r0 + n].to(torch.float64)
        parts.append(torch.stack([rows[:, h * khs:h * khs + D] for h in range(kv_heads)], dim=1))
    return torch.cat(parts)


def scores_of(q, keys, G, scale, mode):
    """q [H, D] float64, keys [L, KV, D] float64 -> (scores [H, L] float64 rounded as ``mode`` says, sum_d |q_d k_jd| [H, L]).
    Mode 1 rounds bf16(bf16(acc) * scale) with fp32 arithmetic: the caller feeds exactly summable inputs, so acc is exact."""
    kh = keys.repeat_interleave(G, dim=1)                         # [L, H, D]
    acc = torch.einsum("hd,lhd->hl", q, kh)
    mag = torch.einsum("hd,lhd->hl", q.abs(), kh.abs())
    if mode == 1:
        a32 = acc.to(torch.float32)
        assert torch.equal(a32.to(torch.float64), acc), "mode 1 needs exactly summable inputs"
        s = (a32.to(torch.bfloat16).to(torch.float32) * np.float32(scale)).to(torch.bfloat16).to(torch.float64)
    else:
        s = acc * float(np.float32(scale))
    return s, mag


def reference(q, tensors, ranges, edges, G, D, scale, mode, khs=None, ld_mass=None):
    """-> (mass [nq, H, ld_mass] float64, bound [nq, H, 1] float64, sum_bound [nq, H]).
    q: [nq, H, D] bf16 (host); per query ``ranges`` [(tensor, row0, rows)] and ``edges``.
    bound: |got - ref| <= bound * ref + 1e-7 with bound = 2 (eps_s + eps_sum + 2^-22),
      eps_s = 2 scale D 2^-24 max_j sum_d |q_d k_jd|  (fp32 accumulation of exact bf16 products, numerator and denominator),
      eps_sum = L 2^-24 (the fp32 sums, worst case), 2^-22 for v_exp_f32; the factor 2 is the margin for second-order terms."""
    nq, H, _ = q.shape
    KV = H // G
    khs = D if khs is None else khs
    nb_max = max(len(e) - 1 for e in edges)
    ld_mass = nb_max if ld_mass is None else ld_mass
    mass = torch.zeros(nq, H, ld_mass, dtype=torch.float64)
    bound = torch.zeros(nq, H, 1, dtype=torch.float64)
    sum_bound = torch.zeros(nq, H, dtype=torch.float64)
    for i in range(nq):
        keys = gather_keys(tensors, ranges[i], KV, D, khs)
        L = keys.shape[0]
        assert edges[i][0] == 0 and edges[i][-1] == L
        s, mag = scores_of(q[i].to(torch.float64), keys, G, scale, mode)
        p = torch.softmax(s, dim=1)
        for b in range(len(edges[i]) - 1):
            mass[i, :, b] = p[:, edges[i][b]:edges[i][b + 1]].sum(dim=1)
        eps_s = 2.0 * float(np.float32(scale)) * D * 2.0 ** -24 * mag.max(dim=1).values
        eps_sum = L * 2.0 ** -24
        bound[i, :, 0] = 2.0 * (eps_s + eps_sum + 2.0 ** -22)
        sum_bound[i] = 2.0 * (eps_sum + 2.0 ** -22)
    return mass, bound, sum_bound


def check(got, ref, bound, what, factor=1.0, extra=0.0):
    """asserts |got - ref| <= factor (bound ref + 1e-7) + extra elementwise; prints the measured maximum next to the bound"""
    got = got.to(torch.float64).cpu()
    err = (got - ref).abs()
    tol = factor * (bound * ref + 1e-7) + extra
    worst = (err / tol).max().item()
    rel = (err / (ref + 1e-30))[ref > 1e-4]
    print(f"{what}: max |got - ref| = {err.max().item():.3e}, max relative (ref > 1e-4) = {rel.max().item() if rel.numel() else 0.0:.3e}, "
          f"relative bound {factor * bound.min().item():.3e} .. {factor * bound.max().item():.3e}, worst error / tolerance = {worst:.3f}")
    assert worst <= 1.0, f"{what}: error / tolerance = {worst:.3f}"
    return worst
