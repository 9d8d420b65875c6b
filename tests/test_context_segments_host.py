"""Segmented contexts (mjv_attn_ctx_segments, include/mjv.h) as far as a CPU can hold them: the host-side planner of
mjv_attention_ctx_seg_bf16 - with no segments it is the plain planner int for int; with segments every part lies in one use,
a tile's parts ascend by key and cover every use once, a context's cuts do not depend on its neighbours, the workspace
follows the part count - the ctypes mirror's layout, and every refusal with its code and the index it names."""
import ctypes as C

import numpy as np
import pytest

from mj_video_amd import _lib
from test_context_any_length_host import KB, TR, Plan, lib, plan_of  # noqa: F401  (lib: the module's fixture)

A, B, CC = 0, 1, 2
OWN = [1, 17, 70]
GEOMS = [(8, 8), (4, 1), (16, 8)]
# (contexts as lists of (tensor, use_len); context_index of the three sequences; tensors)
TWO = [[(A, 100), (B, 37)]]
THREE = [[(A, 64), (B, 1), (CC, 200)]]
CUT = [[(A, 1056), (B, 1000), (CC, 56)]]


def i32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.int32))


def seg_plan(lib, own, index, ctxs, H, G, n_tensors=None, any_length=1, q_lens=None, D=128, cu_ctx=None, raw=None):
    """plan of a segmented launch: (ints or code, workspace bytes or message, plan or None).  ``ctxs`` None: seg == NULL with
    ``cu_ctx``; ``raw``: (cu_use, use_tensor, use_len, n_uses, n_tensors) as given, unchecked."""
    arrs = [i32(np.concatenate([[0], np.cumsum(own)])), i32(index)]
    if cu_ctx is None:
        cu_ctx = np.concatenate([[0], np.cumsum([sum(n for _, n in c) for c in ctxs])])
    arrs.append(i32(cu_ctx))
    q = None if q_lens is None else i32(np.concatenate([[0], np.cumsum(q_lens)]))
    d = _lib.AttnCtxDesc()
    d.cu_seqlens, d.context_index, d.cu_context = (a.ctypes.data for a in arrs)
    d.cu_seqlens_q = None if q is None else q.ctypes.data
    d.n_seqs, d.n_contexts, d.n_heads, d.kv_group, d.head_dim, d.causal = len(index), len(arrs[2]) - 1, H, G, D, 1
    d.ctx_any_length = any_length
    sg, keep = None, None
    if raw is not None or ctxs is not None:
        if raw is None:
            flat = [u for c in ctxs for u in c]
            raw = (np.concatenate([[0], np.cumsum([len(c) for c in ctxs])]), [t for t, _ in flat], [n for _, n in flat], len(flat),
                   n_tensors if n_tensors is not None else max(t for t, _ in flat) + 1)
        keep = [None if a is None else i32(a) for a in raw[:3]]
        sg = _lib.AttnCtxSegments()
        sg.cu_use, sg.use_tensor, sg.use_len = (None if a is None else a.ctypes.data for a in keep)
        sg.n_uses, sg.n_tensors = raw[3], raw[4]
    n = lib.mjv_attention_ctx_seg_plan(C.byref(d), sg, None, 0)
    if n < 0:
        assert lib.mjv_attention_ctx_seg_workspace_bytes(C.byref(d), sg) == n, "the workspace query refuses what the plan refuses"
        return int(n), lib.mjv_last_error().decode(), None
    host = np.empty(n, dtype=np.int32)
    assert lib.mjv_attention_ctx_seg_plan(C.byref(d), sg, host.ctypes.data, n) == n
    return int(n), int(lib.mjv_attention_ctx_seg_workspace_bytes(C.byref(d), sg)), host


def uses_of(p, t, ctx):
    """the parts of context tile ``t`` grouped by use: walks the uses in key order and takes each one's pieces; asserts that
    every part lies in one use, that a use's pieces ascend from 0 to use_len without gap or overlap, that only a use's last
    piece may end off a key-tile boundary and that the fourth int names the use's tensor"""
    ps = [tuple(int(x) for x in r) for r in p.pieces(t)]
    i, out = 0, []
    for tensor, n in ctx:
        at, mine = 0, []
        while at < n:
            assert i < len(ps), f"tile {t}: the parts end before use ({tensor}, {n}) is covered"
            tt, k0, k1, e = ps[i]
            assert tt == t and e == tensor and k0 == at and at < k1 <= n, (t, ps[i], (tensor, n), at)
            assert k0 % KB == 0 and (k1 % KB == 0 or k1 == n)
            mine.append((k0, k1))
            at, i = k1, i + 1
        out.append(mine)
    assert i == len(ps), f"tile {t}: parts behind the last use"
    return out


@pytest.mark.parametrize("H,G", GEOMS)
@pytest.mark.parametrize("ctxs", [TWO, THREE, CUT], ids=["100+37", "64+1+200", "1056+1000+56"])
def test_parts_lie_in_one_use_ascend_and_cover_every_use_once(lib, ctxs, H, G):
    for own, q_lens in ((OWN, None), (OWN, [1, 3, 7]), ([5], [1])):
        index = [0] * len(own)
        n, ws, plan = seg_plan(lib, own, index, ctxs, H, G, q_lens=q_lens)
        assert plan is not None, ws
        p = Plan(plan, G)
        assert ws == p.n_parts * (H // G) * TR * (128 + 2) * 4, "the workspace follows the part count"
        total = sum(n_ for _, n_ in ctxs[0])
        ctx_tiles = [t for t in range(p.n_tiles) if p.tiles[t, 0] == 0]
        assert ctx_tiles == list(range(len(ctx_tiles))) and len(ctx_tiles) == -(-sum(q_lens or own) // p.QS)
        first = None
        for t in ctx_tiles:
            assert p.tiles[t, 2] == total and p.tiles[t, 6] == 0
            got = uses_of(p, t, ctxs[0])
            assert p.tiles[t, 4] == sum(len(u) for u in got)
            first = first or got
            assert got == first, "every tile of a context is cut alike"
        # the cut rule: the chunk follows from the context's tile total and query count as for a plain context
        kt = sum(-(-n_ // KB) for _, n_ in ctxs[0])
        want = max(1, min(-(-512 // (len(ctx_tiles) * (H // G))), 64, max(1, kt // 2)))
        chunk = -(-kt // want) * KB
        for (tensor, n_), mine in zip(ctxs[0], first):
            assert mine == [(k0, min(n_, k0 + chunk)) for k0 in range(0, n_, chunk)]
        # own tiles are those of the plain plan
        _, _, plain = seg_plan(lib, own, index, None, H, G, q_lens=q_lens, cu_ctx=[0, total])
        q = Plan(plain, G)
        own_s, own_p = [t for t in range(p.n_tiles) if p.tiles[t, 0]], [t for t in range(q.n_tiles) if q.tiles[t, 0]]
        assert len(own_s) == len(own_p)
        for a, b in zip(own_s, own_p):
            assert np.array_equal(p.pieces(a)[:, 1:], q.pieces(b)[:, 1:]) and np.array_equal(p.tiles[a, [0, 1, 2, 4, 5]], q.tiles[b, [0, 1, 2, 4, 5]])
        assert np.array_equal(p.rowq[own_s], q.rowq[own_p]) and np.array_equal(p.rowpos[own_s], q.rowpos[own_p])


def test_the_cut_context_is_cut_inside_every_use(lib):
    """1056 + 1000 + 56 keys under one query, one kv head: 17 + 16 + 1 key tiles -> 17 pieces wanted -> chunks of 128 keys;
    9 + 8 + 1 pieces, the last of each use ragged where the use is"""
    _, _, plan = seg_plan(lib, [1], [0], CUT, 8, 8)
    p = Plan(plan, 8)
    got = uses_of(p, 0, CUT[0])
    assert [len(u) for u in got] == [9, 8, 1]
    assert got[0][-1] == (1024, 1056) and got[1][-1] == (896, 1000) and got[2] == [(0, 56)]


@pytest.mark.parametrize("H,G", GEOMS)
def test_walking_a_segmented_plan_gives_the_softmax_over_the_concatenated_keys(lib, H, G):
    """the any-length test's fp64 walk, on the keys as the parts address them: a part's keys are rows [first, end) of ITS
    tensor; merged in plan order they must give the softmax over [use 0 | use 1 | ... | own rows up to the query]"""
    g = np.random.default_rng(5)
    E = 4
    for ctxs in (TWO, THREE, CUT):
        own, q_lens = OWN, [1, 3, 70]
        _, _, plan = seg_plan(lib, own, [0, 0, 0], ctxs, H, G, q_lens=q_lens)
        p = Plan(plan, G)
        tk = {t: g.standard_normal((n + 9, E)) for t, n in ctxs[0]}     # (+ 9 rows behind use_len that nobody may read)
        tv = {t: g.standard_normal((n + 9, E)) for t, n in ctxs[0]}
        cu, cu_q = np.concatenate([[0], np.cumsum(own)]), np.concatenate([[0], np.cumsum(q_lens)])
        q, k, v = g.standard_normal((cu_q[-1], E)), g.standard_normal((cu[-1], E)), g.standard_normal((cu[-1], E))
        ck = np.concatenate([tk[t][:n] for t, n in ctxs[0]])
        cv = np.concatenate([tv[t][:n] for t, n in ctxs[0]])
        for s, (L, lq) in enumerate(zip(own, q_lens)):
            for i in range(lq):
                row, pos = cu_q[s] + i, L - lq + i
                kk, vv = np.concatenate([ck, k[cu[s]:cu[s] + pos + 1]]), np.concatenate([cv, v[cu[s]:cu[s] + pos + 1]])
                sc = kk @ q[row]
                w = np.exp(sc - sc.max())
                want = (w / w.sum()) @ vv
                states = []
                for kind in (0, 1):
                    t = int(p.qinfo[row, kind]) // p.QS
                    for _, k0, k1, e in p.pieces(t):
                        if kind == 0:
                            keys, vals = tk[int(e)][k0:k1], tv[int(e)][k0:k1]
                        else:
                            hi = min(k1, pos + 1)
                            keys, vals = k[cu[s] + k0:cu[s] + hi], v[cu[s] + k0:cu[s] + hi]
                        sp = keys @ q[row]
                        ex = np.exp(sp - sp.max())
                        states.append((sp.max(), ex.sum(), ex @ vals))
                m = max(st[0] for st in states)
                l = sum(st[1] * np.exp(st[0] - m) for st in states)
                o = sum(st[2] * np.exp(st[0] - m) for st in states)
                assert np.abs(o / l - want).max() < 1e-9


PLAIN = [([0, 5], [0], [0, 100]), ([0, 1, 18, 88], [0, 0, 0], [0, 137]), ([0, 1, 18, 88], [0, 1, 0], [0, 2112, 2249]),
         ([0, 1, 18, 88], [1, 1, 0], [0, 64, 64 + 28672])]


@pytest.mark.parametrize("H,G", GEOMS + [(16, 2)])
def test_no_segments_is_the_plain_plan_int_for_int(lib, H, G):
    for cu_seq, index, cu_ctx in PLAIN:
        own = np.diff(cu_seq).tolist()
        for q_lens in (None, [1] * len(own)):
            cu_q = None if q_lens is None else np.concatenate([[0], np.cumsum(q_lens)])
            a = plan_of(lib, cu_seq, index, cu_ctx, H=H, G=G, cu_q=cu_q)
            b = seg_plan(lib, own, index, None, H, G, q_lens=q_lens, cu_ctx=cu_ctx)
            assert a[0] == b[0] and a[1] == b[1] and np.array_equal(a[2], b[2])


@pytest.mark.parametrize("H,G", GEOMS)
@pytest.mark.parametrize("length", [1, 64, 100, 137, 2112, 2149, 28672])
def test_one_use_is_the_plain_plan_but_for_the_fourth_int(lib, length, H, G):
    for q_lens in (None, [1, 2, 3]):
        n, ws, plain = seg_plan(lib, OWN, [0, 0, 0], None, H, G, q_lens=q_lens, cu_ctx=[0, length])
        n2, ws2, seg = seg_plan(lib, OWN, [0, 0, 0], [[(3, length)]], H, G, n_tensors=5, q_lens=q_lens)
        assert (n, ws) == (n2, ws2)
        p, s = Plan(plain, G), Plan(seg, G)
        ctx_parts = np.isin(s.parts[:, 0], np.flatnonzero(s.tiles[:, 0] == 0))
        assert (s.parts[ctx_parts, 3] == 3).all() and (s.parts[~ctx_parts, 3] == 0).all() and (p.parts[:, 3] == 0).all()
        same = seg.copy()
        Plan(same, G).parts[:, 3] = 0
        assert np.array_equal(same, plain)


@pytest.mark.parametrize("H,G", GEOMS)
def test_a_context_is_cut_the_same_alone_and_in_company(lib, H, G):
    """independence: context 0 = [(A,100),(B,37)] keeps its parts when a second context joins the launch - one
    that shares tensor A, with sequences of its own interleaved"""
    alone = Plan(seg_plan(lib, OWN, [0, 0, 0], TWO, H, G)[2], G)
    for second in ([(A, 100), (CC, 2000)], [(A, 64)], [(CC, 700), (A, 100), (B, 37)]):
        own = [OWN[0], 9, OWN[1], 200, OWN[2]]
        both = Plan(seg_plan(lib, own, [0, 1, 0, 1, 0], [TWO[0], second], H, G)[2], G)
        mine = [t for t in range(both.n_tiles) if both.tiles[t, 0] == 0 and both.tiles[t, 6] == 0]
        theirs = [t for t in range(alone.n_tiles) if alone.tiles[t, 0] == 0]
        assert len(mine) == len(theirs) > 0
        for t, u in zip(mine, theirs):
            assert np.array_equal(both.tiles[t, [2, 4, 5]], alone.tiles[u, [2, 4, 5]])
            assert np.array_equal(both.pieces(t)[:, 1:], alone.pieces(u)[:, 1:])
        for t in range(both.n_tiles):
            if both.tiles[t, 0] == 0 and both.tiles[t, 6] == 1:
                uses_of(both, t, second)


def test_ctypes_struct_has_the_documented_layout():
    S = _lib.AttnCtxSegments
    assert [f[0] for f in S._fields_] == ["cu_use", "use_tensor", "use_len", "n_uses", "n_tensors"]
    assert [getattr(S, f[0]).offset for f in S._fields_] == [0, 8, 16, 24, 28] and C.sizeof(S) == 32
    # the descriptor itself is untouched
    assert C.sizeof(_lib.AttnCtxDesc()) == 240 == _lib._ATTN_CTX_DESC_BYTES and _lib.ABI_VERSION == 7
    for name in ("mjv_attention_ctx_seg_plan", "mjv_attention_ctx_seg_workspace_bytes", "mjv_attention_ctx_seg_bf16"):
        assert name in _lib.SYMBOLS


def test_refusals(lib):
    own, index = [5], [0]
    cases = [
        (dict(ctxs=[[(A, 100), (B, 37)]], any_length=0), -1, "use 0 has 100 keys"),
        (dict(ctxs=[[(A, 128), (B, 37)]], any_length=0), -1, "use 1 has 37 keys"),
        (dict(ctxs=[[(A, 100), (B, 0)]]), -1, "use 1 has 0 keys"),
        (dict(ctxs=[[(A, 100), (B, -3)]]), -1, "use 1 has -3 keys"),
        (dict(ctxs=[[(A, 100), (2, 37)]], n_tensors=2), -1, "use 1 names tensor 2 of 2"),
        (dict(ctxs=[[(-1, 100), (B, 37)]], n_tensors=2), -1, "use 0 names tensor -1 of 2"),
        (dict(ctxs=[[(A, 100), (B, 37)]], cu_ctx=[0, 138]), -1, "context 0 has 138 keys, its uses add up to 137"),
        (dict(ctxs=[[(A, 100), (B, 37)]], D=96), -3, "head_dim 96"),
        (dict(ctxs=[[(A, 100), (B, 37)]], any_length=2), -1, "ctx_any_length"),
        (dict(ctxs=None, cu_ctx=[0, 137], raw=([0, 0], [0], [137], 1, 1)), -1, "cu_use"),
        (dict(ctxs=None, cu_ctx=[0, 137], raw=([0, 1], [0, 0], [137, 5], 2, 1)), -1, "cu_use"),
        (dict(ctxs=None, cu_ctx=[0, 137], raw=(None, [0], [137], 1, 1)), -1, "null segment array"),
        (dict(ctxs=None, cu_ctx=[0, 137], raw=([0, 1], [0], [137], 1, 0)), -1, "0 tensors"),
    ]
    for kw, code, text in cases:
        rc, msg, _ = seg_plan(lib, own, index, kw.pop("ctxs"), 4, 2, **kw)
        assert rc == code and text in msg, (kw, rc, msg)
    # the second context of a launch: the message names it
    rc, msg, _ = seg_plan(lib, [5, 5], [0, 1], [[(A, 64)], [(A, 64), (B, 10)]], 4, 2, cu_ctx=[0, 64, 139])
    assert rc == -1 and "context 1 has 75 keys, its uses add up to 74" in msg
    rc, msg, _ = seg_plan(lib, [5, 5], [0, 1], None, 4, 2, cu_ctx=[0, 64, 138], raw=([0, 1, 1], [0], [64], 1, 1))
    assert rc == -1 and "context 1 has no use" in msg
    assert seg_plan(lib, own, index, [[(A, 128), (B, 64)]], 4, 2, any_length=0)[2] is not None
    assert seg_plan(lib, own, index, [[(A, 100), (B, 37)]], 4, 2)[2] is not None


def test_packed_rows_with_segments_are_refused_before_anything_is_launched(lib):
    """the launch entry's own rule: segments travel with ctx_k_list / ctx_v_list.  Host-side: the pointers are never followed
    (a refusal comes before any launch), so placeholders do"""
    keep = [i32([0, 5]), i32([0]), i32([0, 137]), i32([0, 2]), i32([0, 1]), i32([100, 37])]
    d = _lib.AttnCtxDesc()
    d.cu_seqlens, d.context_index, d.cu_context = (a.ctypes.data for a in keep[:3])
    d.n_seqs, d.n_contexts, d.n_heads, d.kv_group, d.head_dim, d.causal, d.ctx_any_length = 1, 1, 4, 2, 128, 1, 1
    d.Q = d.K = d.V = d.O = d.ctx_k = d.ctx_v = 0x1000
    sg = _lib.AttnCtxSegments()
    sg.cu_use, sg.use_tensor, sg.use_len = (a.ctypes.data for a in keep[3:])
    sg.n_uses, sg.n_tensors = 2, 2
    assert lib.mjv_attention_ctx_seg_bf16(C.byref(d), C.byref(sg), None) == -1
    assert "segments need the pointer lists" in lib.mjv_last_error().decode()
    d.ctx_k_list = 0x1000   # one list without the other
    assert lib.mjv_attention_ctx_seg_bf16(C.byref(d), C.byref(sg), None) == -1
    assert "both be given" in lib.mjv_last_error().decode()


def test_ops_plan_takes_segments_and_checks_the_tensors_per_use():
    """``ops.AttnCtxPlan(segments=...)`` / ``ops._check_ctx_rows`` on CPU tensors (attributes only): a tensor needs the rows of
    the longest use that names it, not more"""
    import torch
    from mj_video_amd import ops
    plan = ops.AttnCtxPlan([0, 5], [0], [0, 137], 4, 2, 128, "cpu", any_length=True, segments=[[(0, 100), (1, 37)]])
    plain = ops.AttnCtxPlan([0, 5], [0], [0, 137], 4, 2, 128, "cpu", any_length=True)
    assert plan.segmented and not plain.segmented and plain.seg_desc() is None and plan.n_tensors == 2
    assert plan.workspace_bytes * 2 == plain.workspace_bytes * 3 and plan.plan_ints == plain.plan_ints + 4   # 3 parts for 2
    dev = torch.device("cpu")
    t = lambda rows: torch.zeros(rows, 256, dtype=torch.bfloat16)  # noqa: E731
    assert ops._check_ctx_rows([t(100), t(37)], [t(120), t(40)], plan, dev, 128, 128) == (256, 256)
    with pytest.raises(ValueError, match=r"segment tensor 1 \(keys\): 36 rows, the longest use of it reads 37"):
        ops._check_ctx_rows([t(100), t(36)], [t(100), t(37)], plan, dev, 128, 128)
    with pytest.raises(ValueError, match="3 key / 2 value tensors for the plan's 2 segment tensors"):
        ops._check_ctx_rows([t(100), t(37), t(1)], [t(100), t(37)], plan, dev, 128, 128)
    shared = ops.AttnCtxPlan([0, 5, 9], [0, 1], [0, 137, 201], 4, 2, 128, "cpu", any_length=True,
                             segments=[[(0, 100), (1, 37)], [(0, 64)]])
    assert shared.n_tensors == 2 and shared.cu_use.tolist() == [0, 2, 3]
    with pytest.raises(_lib.MjvLibraryError, match=r"\(-1\).*of 0 tensors"):
        ops.AttnCtxPlan([0, 5, 9], [0, 1], [0, 137, 201], 4, 2, 128, "cpu", any_length=True,
                        segments=[[(0, 100), (1, 37)], [(0, 64)]], n_tensors=0)
    with pytest.raises(ValueError, match="segments for 1 contexts"):
        ops.AttnCtxPlan([0, 5, 9], [0, 1], [0, 137, 201], 4, 2, 128, "cpu", any_length=True, segments=[[(0, 201)]])


def test_extend_context_analysis_and_segment_bookkeeping_need_no_gpu():
    """``model._analyse_extension`` (ids, lengths, where every new row's image embedding comes from) and what a ``VideoContext``
    says of its segments, on CPU tensors: the first two tiles of the tiny one-video case under their own prompt (64 tokens: the
    context ends before the image run, all 8 image tokens wait in ``img_tail``), extended by the other two"""
    import torch
    import captions_util as cu
    from mj_video_amd import synth
    from mj_video_amd.modeling import InternVLChatRewardModeling, VideoContext
    cfg, videos, prompts, _ = cu.one_case("tiny")
    model = InternVLChatRewardModeling.from_config(cfg, dtype=torch.bfloat16)
    model.config.pad_token_id = synth.PAD_ID
    model.model.img_context_token_id = synth.IMG_CONTEXT_ID
    px = videos[0].to(torch.bfloat16)
    a = model._analyse_video(px[:2], synth.synth_input_ids(8, 500, n_caption=1))
    assert (a["P"], a["n_in"], a["n_img"]) == (64, 0, 8)
    cpu = torch.device("cpu")
    rows = lambda n: [torch.full((n, 8), float(n), dtype=torch.bfloat16) for _ in range(2)]  # noqa: E731  (two layers)
    parent = VideoContext(a["ids"], 64, rows(64), rows(64), torch.zeros(8, 4, dtype=torch.bfloat16), a["cols"].copy(), 8, None, None, 0, cpu)
    assert len(parent.segments) == 1 and parent.segments[0][0] is parent.k and parent.segments[0][2] == 64
    assert parent.nbytes == parent.storage_nbytes == (2 * 2 * 64 * 8 + 8 * 4) * 2
    full = prompts[0]
    first = int(np.flatnonzero(full[0].numpy() == synth.IMG_CONTEXT_ID)[0])
    assert first == 71
    for K, n_in in ((65, 0), (71, 0), (72, 1), (80, 9), (87, 16), (117, 16)):
        e = model._analyse_extension(parent, full, px[2:], context_len=K)
        assert (e["K"], e["n_in0"], e["n_in"], e["n_new"]) == (K, 0, n_in, 8) and e["src"].shape == (K - 64,)
        want = np.full(K - 64, -1)
        want[first - 64:first - 64 + n_in] = np.arange(n_in)     # embedding j of [parent's tail | new tiles] at image token j
        assert np.array_equal(e["src"], want) and np.array_equal(e["new_ids"], full[0, 64:K].numpy())
    with pytest.raises(ValueError, match="would hold 64 tokens, the context to extend holds 64 already"):
        model._analyse_extension(parent, full, px[2:])
    with pytest.raises(ValueError, match="pixel_values holds 0 new tiles"):
        model._analyse_extension(parent, full, context_len=80)
    bad = full.clone()
    bad[0, 63] += 1
    with pytest.raises(ValueError, match=r"first at column 63"):
        model._analyse_extension(parent, bad, px[2:], context_len=80)
    # a child holds its parent's lists by reference, its own rows last; clone() is plain and owns one run of rows
    child = VideoContext(full[0, :80].numpy(), 80, rows(16), rows(16), torch.zeros(7, 4, dtype=torch.bfloat16), np.arange(80, 87), 16, None,
                         None, 0, cpu, base=parent.segments)
    grand = VideoContext(full[0, :117].numpy(), 117, rows(37), rows(37), torch.zeros(0, 4, dtype=torch.bfloat16), np.arange(0), 16, None,
                         None, 0, cpu, base=child.segments)
    assert [n for _, _, n in grand.segments] == [64, 16, 37] and grand.segments[0][0] is parent.k and grand.segments[1][1] is child.v
    assert grand.nbytes == 2 * 2 * 37 * 8 * 2 and grand.storage_nbytes == 2 * 2 * 117 * 8 * 2
    assert child.nbytes == (2 * 2 * 16 * 8 + 7 * 4) * 2 and child.storage_nbytes == child.nbytes + 2 * 2 * 64 * 8 * 2
    flat = grand.clone()
    assert len(flat.segments) == 1 and flat.P == 117 and flat.k[1].shape == (117, 8) and flat.nbytes == flat.storage_nbytes == grand.storage_nbytes
    assert flat.k[0][:, 0].tolist() == [64.0] * 64 + [16.0] * 16 + [37.0] * 37
