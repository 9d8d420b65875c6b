"""Video contexts of any length, as far as a CPU can hold them: the host-side planner of mjv_attention_ctx_bf16 with
``ctx_any_length`` (coverage, cut rule, masks - walked in numpy against a direct softmax), its refusals,
``harness.shared_prefix_len`` on the project's own test prompts, and the ``context_len`` argument checks of the model."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import captions_util as cu
from mj_video_amd import _lib, harness, synth

TR, KB = 128, 64
RAGGED = (1, 31, 32, 33, 63, 65, 100, 127, 129, 613, 2149)


@pytest.fixture(scope="module")
def lib():
    if not os.path.isfile(_lib.LIB_PATH):
        _lib.build_library()
    return _lib.load_library()


def plan_of(lib, cu_seq, index, cu_ctx, H=16, G=2, D=128, cu_q=None, any_length=1):
    arrs = [np.ascontiguousarray(np.asarray(a, dtype=np.int32)) for a in (cu_seq, index, cu_ctx)]
    q = None if cu_q is None else np.ascontiguousarray(np.asarray(cu_q, dtype=np.int32))
    d = _lib.AttnCtxDesc()
    d.cu_seqlens, d.context_index, d.cu_context = (a.ctypes.data for a in arrs)
    d.cu_seqlens_q = None if q is None else q.ctypes.data
    d.n_seqs, d.n_contexts, d.n_heads, d.kv_group, d.head_dim, d.causal = len(arrs[1]), len(arrs[2]) - 1, H, G, D, 1
    d.ctx_any_length = any_length
    n = lib.mjv_attention_ctx_plan(C.byref(d), None, 0)
    if n < 0:
        return int(n), lib.mjv_last_error().decode(), None
    host = np.empty(n, dtype=np.int32)
    assert lib.mjv_attention_ctx_plan(C.byref(d), host.ctypes.data, n) == n
    return int(n), int(lib.mjv_attention_ctx_workspace_bytes(C.byref(d))), host


class Plan:
    """the sections of a plan (csrc/attention.hip, namespace cx: header | parts | tiles | rowq | rowpos | qinfo)"""

    def __init__(self, plan, G):
        self.n_parts, self.n_tiles, self.total_q = (int(x) for x in plan[1:4])
        assert int(plan[4]) == G
        self.QS = TR // G
        o = 8
        self.parts = plan[o:o + 4 * self.n_parts].reshape(-1, 4)
        o += 4 * self.n_parts
        self.tiles = plan[o:o + 8 * self.n_tiles].reshape(-1, 8)
        o += 8 * self.n_tiles
        self.rowq = plan[o:o + self.n_tiles * self.QS].reshape(self.n_tiles, self.QS)
        o += self.n_tiles * self.QS
        self.rowpos = plan[o:o + self.n_tiles * self.QS].reshape(self.n_tiles, self.QS)
        o += self.n_tiles * self.QS
        self.qinfo = plan[o:o + 2 * self.total_q].reshape(self.total_q, 2)

    def pieces(self, t):
        return self.parts[self.tiles[t, 3]:self.tiles[t, 3] + self.tiles[t, 4]]


def own_lengths(n, seed):
    g = np.random.default_rng(seed)
    lens = g.integers(1, 201, size=n).tolist()
    lens[0] = 1
    if n > 1:
        lens[-1] = 200
    return lens


def launch(ctx_lens, n, suffix, seed):
    own = own_lengths(n, seed)
    index = [i % len(ctx_lens) for i in range(n)]
    q_lens = [min(L, 1 + (i * 3) % 7) for i, L in enumerate(own)] if suffix else list(own)
    return own, index, q_lens


def check_pieces(p, ctx_lens):
    for t in range(p.n_tiles):
        kind, _, nkeys, _, nsplit, _, c = (int(x) for x in p.tiles[t, :7])
        ps = p.pieces(t)
        assert (ps[:, 0] == t).all() and ps[0, 1] == 0 and (ps[1:, 1] == ps[:-1, 2]).all() and (ps[:, 2] > ps[:, 1]).all()
        if kind == 0:
            assert nkeys == ctx_lens[c], "te[2] is the context's length"
            assert ps[-1, 2] == nkeys, "the last piece ends at the length"
            assert (ps[:-1, 2] % KB == 0).all() and (ps[:, 1] % KB == 0).all(), "every other piece is whole tiles"
            assert nsplit <= max(1, -(-nkeys // KB) // 2), "pieces of at least two key tiles"


def walk(p, G, own, index, q_lens, ctx_lens, seed):
    """every query's attention as the plan lays it out - per piece an online-softmax state (max, sum, weighted values) over the
    piece's keys [first, end), the own piece masked behind the row's position; merged in plan order - against a direct softmax
    over [context | own rows up to the query].  fp64, one head of 4 elements: the plan is the same for every head."""
    g = np.random.default_rng(seed)
    E = 4
    cu, cu_q, cu_c = (np.concatenate([[0], np.cumsum(a)]) for a in (own, q_lens, ctx_lens))
    q = g.standard_normal((cu_q[-1], E))
    k, v = g.standard_normal((cu[-1], E)), g.standard_normal((cu[-1], E))
    ck, cv = g.standard_normal((cu_c[-1], E)), g.standard_normal((cu_c[-1], E))
    seen = np.zeros((p.total_q, 2), int)
    worst = 0.0
    for s, (L, lq) in enumerate(zip(own, q_lens)):
        c = index[s]
        for i in range(lq):
            row = cu_q[s] + i
            pos = L - lq + i
            kk = np.concatenate([ck[cu_c[c]:cu_c[c + 1]], k[cu[s]:cu[s] + pos + 1]])
            vv = np.concatenate([cv[cu_c[c]:cu_c[c + 1]], v[cu[s]:cu[s] + pos + 1]])
            sc = kk @ q[row]
            w = np.exp(sc - sc.max())
            want = (w / w.sum()) @ vv
            states = []
            for kind in (0, 1):
                sl = int(p.qinfo[row, kind])
                t, j = sl // p.QS, sl % p.QS
                assert p.tiles[t, 0] == kind and p.rowq[t, j] == row and j * G < p.tiles[t, 5]
                seen[row, kind] += 1
                for _, k0, k1, _ in p.pieces(t):
                    if kind == 0:
                        assert p.tiles[t, 6] == c and p.tiles[t, 1] == cu_c[c]
                        keys, vals = ck[cu_c[c] + k0:cu_c[c] + k1], cv[cu_c[c] + k0:cu_c[c] + k1]
                    else:
                        assert p.tiles[t, 1] == cu[s] and p.rowpos[t, j] == pos and k1 > pos, "the own piece reaches the row"
                        hi = min(k1, pos + 1)
                        keys, vals = k[cu[s] + k0:cu[s] + hi], v[cu[s] + k0:cu[s] + hi]
                    sp = keys @ q[row]
                    m = sp.max()
                    e = np.exp(sp - m)
                    states.append((m, e.sum(), e @ vals))
            m = max(st[0] for st in states)
            l = sum(st[1] * np.exp(st[0] - m) for st in states)
            o = sum(st[2] * np.exp(st[0] - m) for st in states)
            worst = max(worst, float(np.abs(o / l - want).max()))
    assert (seen == 1).all()
    assert worst < 1e-9, worst


SETS = [[L] for L in RAGGED] + [[33, 64], [2149, 576, 293], [128, 1, 613], [63, 65, 2112, 100], list(RAGGED[:6]), list(RAGGED[5:])]


@pytest.mark.parametrize("H", [4, 16])
@pytest.mark.parametrize("ctx_lens", SETS, ids=lambda s: "-".join(map(str, s)))
def test_ragged_plan_covers_every_key_once(lib, ctx_lens, H):
    """flag on: every context's pieces are ascending, disjoint and cover [0, len); only a context's last piece may end off a
    tile boundary; walking the plan gives the softmax over [context | own].  1 - 7 sequences, all own rows or suffix queries."""
    G = 2
    for n in sorted({1, 2, 5, 7, max(1, len(ctx_lens))}):
        if n < len(ctx_lens) and n != 1:
            continue   # (n = 1 keeps the case of contexts that no sequence names)
        for suffix in (False, True):
            own, index, q_lens = launch(ctx_lens, n, suffix, seed=n + len(ctx_lens))
            cu_seq, cu_q = np.concatenate([[0], np.cumsum(own)]), np.concatenate([[0], np.cumsum(q_lens)])
            cu_ctx = np.concatenate([[0], np.cumsum(ctx_lens)])
            n_ints, ws, plan = plan_of(lib, cu_seq, index, cu_ctx, H=H, G=G, cu_q=cu_q if suffix else None)
            assert plan is not None, ws
            p = Plan(plan, G)
            assert ws == p.n_parts * (H // G) * TR * (128 + 2) * 4 and p.total_q == sum(q_lens)
            check_pieces(p, ctx_lens)
            if H == 4 or n <= 2:   # (the walk does not depend on H beyond the cut points: the long ones once per shape)
                walk(p, G, own, index, q_lens, ctx_lens, seed=7)


@pytest.mark.parametrize("ctx_lens", [[64], [2112], [2112, 576], [576, 2112, 64], [28672], [128, 1536, 64]])
def test_whole_tile_lengths_plan_as_with_the_flag_off(lib, ctx_lens):
    for n in (1, 5, 7):
        for suffix in (False, True):
            own, index, q_lens = launch(ctx_lens, n, suffix, seed=n)
            args = (np.concatenate([[0], np.cumsum(own)]), index, np.concatenate([[0], np.cumsum(ctx_lens)]))
            kw = dict(cu_q=np.concatenate([[0], np.cumsum(q_lens)]) if suffix else None)
            for H in (4, 16):
                on, off = plan_of(lib, *args, H=H, any_length=1, **kw), plan_of(lib, *args, H=H, any_length=0, **kw)
                assert on[0] == off[0] and on[1] == off[1] and np.array_equal(on[2], off[2])


def test_a_ragged_context_is_cut_the_same_alone_and_in_company(lib):
    G = 2
    own, q_lens = own_lengths(7, 3), None
    index = [0, 1, 0, 2, 1, 0, 2]
    ctx_lens = [2149, 576, 613]
    _, _, plan = plan_of(lib, np.concatenate([[0], np.cumsum(own)]), index, np.concatenate([[0], np.cumsum(ctx_lens)]), G=G)
    p = Plan(plan, G)
    for c, L in enumerate(ctx_lens):
        keep = [i for i, x in enumerate(index) if x == c]
        _, _, alone = plan_of(lib, np.concatenate([[0], np.cumsum([own[i] for i in keep])]), [0] * len(keep), [0, L], G=G)
        a = Plan(alone, G)
        mine = [t for t in range(p.n_tiles) if p.tiles[t, 0] == 0 and p.tiles[t, 6] == c]
        theirs = [t for t in range(a.n_tiles) if a.tiles[t, 0] == 0]
        assert len(mine) == len(theirs) > 0
        for t, u in zip(mine, theirs):
            assert p.tiles[t, 4] == a.tiles[u, 4] and p.tiles[t, 5] == a.tiles[u, 5] and p.tiles[t, 2] == a.tiles[u, 2] == L
            assert np.array_equal(p.pieces(t)[:, 1:3], a.pieces(u)[:, 1:3])


def test_refusals(lib):
    for args, kw, code, text in [
        (([0, 5], [0], [0, 100]), dict(any_length=0), -1, "multiple of 64"),
        (([0, 5], [0], [0, 0]), dict(any_length=1), -1, "context 0 has 0 keys"),
        (([0, 5, 9], [0, 1], [0, 100, 100]), dict(any_length=1), -1, "context 1 has 0 keys"),
        (([0, 5], [0], [0, 100]), dict(any_length=2), -1, "ctx_any_length"),
        (([0, 5], [0], [0, 64]), dict(any_length=2), -1, "ctx_any_length"),
        (([0, 5], [0], [0, 100]), dict(any_length=-1), -1, "ctx_any_length"),
        (([0, 5], [0], [0, 100]), dict(any_length=1, D=96), -3, "head_dim 96"),
        (([0, 5], [0], [0, 100]), dict(any_length=1, D=64), -3, "head_dim 64"),
    ]:
        rc, msg, _ = plan_of(lib, *args, **kw)
        assert rc == code and text in msg, (args, kw, rc, msg)
    rc, _, plan = plan_of(lib, [0, 5], [0], [0, 100], any_length=1)
    assert rc > 0 and plan is not None


def test_descriptor_mirror_carries_the_flag_behind_the_lists(lib):
    """the ctypes mirror: ``_fields_`` still ends with the lists, the instance is as large as the C struct (8 pointers / int64
    pairs ... 232 bytes through ctx_v_list, one int32, padded to 240), a fresh descriptor asks for the old rule, and the C side
    reads the flag where the mirror writes it (length 100: refused at 0, planned at 1, refused at 2)"""
    d = _lib.AttnCtxDesc()
    names = [f[0] for f in _lib.AttnCtxDesc._fields_]
    assert names[-2:] == ["ctx_k_list", "ctx_v_list"] and "ctx_any_length" not in names
    assert _lib.AttnCtxDesc.ctx_v_list.offset + 8 == 232 == _lib._ATTN_CTX_ANY_LENGTH_OFFSET
    assert C.sizeof(d) == 240 == _lib._ATTN_CTX_DESC_BYTES and d.ctx_any_length == 0
    d.ctx_any_length = 1
    d.ctx_v_list = 0x7fff_ffff_ffff
    assert d.ctx_any_length == 1 and d.ctx_v_list == 0x7fff_ffff_ffff, "neighbours do not overlap"
    d.ctx_any_length = -1
    assert d.ctx_any_length == -1
    assert [plan_of(lib, [0, 5], [0], [0, 100], any_length=f)[0] < 0 for f in (0, 1, 2)] == [True, False, True]
    assert _lib.ABI_VERSION == 7


def prompts_per_video(dims, case):
    _, videos, prompts, index = cu.CASES[case](dims)
    return [[prompts[i] for i in np.flatnonzero(index == v)] for v in range(len(videos))]


@pytest.mark.parametrize("dims,case,want", [("tiny", "one", [117]), ("tiny", "multi", [133, 125, 113]),
                                            ("2b", "one", [613]), ("2b", "multi", [613, 485, 293])])
def test_shared_prefix_len_of_the_test_prompts(dims, case, want):
    got = [harness.shared_prefix_len(rows, synth.PAD_ID) for rows in prompts_per_video(dims, case)]
    assert got == want
    assert all(k % 64 for k in got)
    # the same on the right-padded batch the model sees
    for rows, k in zip(prompts_per_video(dims, case), want):
        ids, _ = synth.pad_batch(rows)
        assert harness.shared_prefix_len(list(ids), synth.PAD_ID) == k


def test_shared_prefix_len_keeps_the_selected_rows_outside():
    from mj_video_amd.modeling import find_token_for_gating
    rows = prompts_per_video("tiny", "one")[0]
    twice = [rows[3], rows[3]]
    k = harness.shared_prefix_len(twice, synth.PAD_ID)
    row = rows[3].reshape(-1).numpy()
    r, g = row.shape[0] - 1, find_token_for_gating(row)
    assert k == min(r, g) < row.shape[0], "identical prompts share everything: the cap decides"
    # a long and a short copy of one prompt family: the cap comes from the row that ends first
    for group in (rows, rows[:2], [rows[0]], twice + [rows[5]]):
        k = harness.shared_prefix_len(group, synth.PAD_ID)
        for t in group:
            a = t.reshape(-1).numpy()
            assert k <= a.shape[0] - 1 and k <= find_token_for_gating(a) and k >= 1
            assert all((u.reshape(-1).numpy()[:k] == a[:k]).all() for u in group)
    with pytest.raises(ValueError):
        harness.shared_prefix_len([], synth.PAD_ID)


def test_context_len_argument_checks_need_no_gpu():
    from mj_video_amd.modeling import InternVLChatRewardModeling
    cfg, videos, prompts, index = cu.multi_case("tiny")
    model = InternVLChatRewardModeling.from_config(cfg, dtype=torch.bfloat16)
    model.config.pad_token_id = synth.PAD_ID
    model.model.img_context_token_id = synth.IMG_CONTEXT_ID
    px = [v.to(torch.bfloat16) for v in videos]
    first = [prompts[int(np.flatnonzero(index == v)[0])] for v in range(3)]
    N = first[0].shape[1]
    for bad in (0, N, -1, 64.0, "64", True):
        with pytest.raises(ValueError, match="context_len"):
            model._analyse_video(px[0], first[0], context_len=bad)
    cols = np.flatnonzero(first[0][0].numpy() == synth.IMG_CONTEXT_ID)
    end = int(cols[-1]) + 1
    for K, n_in in ((1, 0), (int(cols[0]) + 5, 5), (end, cols.size), (end + 7, cols.size), (N - 1, cols.size)):
        a = model._analyse_video(px[0], first[0], context_len=K)
        assert a["P"] == K and a["ids"].shape == (K,) and a["n_in"] == n_in
    assert model._analyse_video(px[0], first[0])["P"] == end // 64 * 64 == model._analyse_video(px[0], first[0], context_len=None)["P"]
    am = torch.ones(N, dtype=torch.bool)
    am[end + 2] = False
    model._analyse_video(px[0], first[0], am, context_len=end + 2)
    with pytest.raises(ValueError, match=rf"masked column {end + 2} inside the context \({end + 3} tokens\)"):
        model._analyse_video(px[0], first[0], am, context_len=end + 3)
    # encode_videos: None, one int, one entry per video
    lens = [133, 125, 113]
    info = model._analyse_videos(px, first, context_len=lens)
    assert [v["P"] for v in info["videos"]] == lens and info["cu"].tolist() == [0, 133, 258, 371]
    assert [v["P"] for v in model._analyse_videos(px, first, context_len=70)["videos"]] == [70] * 3
    assert [v["P"] for v in model._analyse_videos(px, first)["videos"]] == [v["P"] for v in model._analyse_videos(px, first, context_len=[None] * 3)["videos"]]
    with pytest.raises(ValueError, match="context_len of 2 entries"):
        model._analyse_videos(px, first, context_len=[64, 64])
    with pytest.raises(ValueError, match="video 1: context_len"):
        model._analyse_videos(px, first, context_len=[64, 0, 64])
    with pytest.raises(ValueError, match="video 0: context_len"):
        model._analyse_videos(px, first, context_len=64.0)
