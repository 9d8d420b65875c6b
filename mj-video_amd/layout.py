"""Token layout: everything the host derives from token ids before a kernel runs - which rows are packed, at which positions,
where image embeddings are spliced in, which two rows per sequence the heads read - and every refusal of a prompt the model cannot
take (nothing is repaired).  Pure functions of numpy arrays and plain values: no tensor, no model, no device; where a tensor's
shape or dtype is checked, the caller passes the shape and the dtype's name (``str(tensor.dtype)``).  Each rule lives once, in a
helper; the analysers are built on the helpers, and the model's ``_analyse_*`` methods convert tensors and delegate."""
from __future__ import annotations

from typing import NamedTuple, Optional, Sequence, Tuple

import numpy as np

# `<|im_end|><|im_start|>assistant\n` in InternLM2 token ids (moe_reward.py:45-48)
token_pattern = [92542, 92543, 525, 11353, 364]


def find_token_for_gating(lst, pattern=None) -> int:
    """Index of the LAST occurrence of ``token_pattern`` in ``lst`` (moe_reward.py:50-57).  ``pattern``: another tokenizer's ids
    of the same marker (``config.gating_token_pattern``: the Phi-3 backbone of BASELINE configs[4]); default = the reference's
    module constant."""
    a = np.asarray(lst)
    pattern = token_pattern if pattern is None else list(pattern)
    n = len(pattern)
    if a.shape[0] >= n:
        hit = np.ones(a.shape[0] - n + 1, dtype=bool)
        for j, t in enumerate(pattern):
            hit &= a[j:a.shape[0] - n + 1 + j] == t
        idx = np.flatnonzero(hit)
        if idx.size:
            return int(idx[-1])
    raise ValueError("Token pattern not found in the list.")


class TokenRules(NamedTuple):
    """what the analysers read from the model and its config.  Of a context (``ctx`` / ``ctxs`` below: a ``VideoContext``, or
    anything with these attributes) they read ``P``, ``ids``, ``n_img`` and ``tail_cols``, all numpy arrays and ints."""
    pad_id: Optional[int]                        # config.pad_token_id
    ctx_id: Optional[int]                        # <IMG_CONTEXT> (model.model.img_context_token_id)
    vocab: int                                   # rows of the token embedding
    tokens_per_tile: int                         # image tokens per tile (model.model.num_image_token)
    gating_pattern: Optional[Sequence[int]]      # config.gating_token_pattern (None: ``token_pattern``)


# ------------------------------------------------------------------------------------------------ the rules, once each
def selected_columns(row: np.ndarray, pad_id, gating_pattern=None) -> Tuple[int, int]:
    """(r, g) of one row of N ids: the reward column - N - 1 without a ``pad_id``, else the column before the first ``pad_id``, modulo N
    (no pad, or one at column 0: N - 1; moe_reward.py:226-237) - and the gating column, where the LAST gating pattern starts."""
    N = row.shape[0]
    r = N - 1 if pad_id is None else (int(np.argmax(row == pad_id)) - 1) % N
    return r, find_token_for_gating(row, gating_pattern)


def normalise_mask(am: Optional[np.ndarray], shape) -> np.ndarray:
    """the attention mask as a bool array of ``shape`` (None: every column valid)"""
    if am is None:
        return np.ones(shape, dtype=bool)
    if am.shape != shape:
        raise ValueError(f"attention_mask shape {am.shape} != input_ids shape {shape}")
    return am.astype(bool)


def check_vocabulary(valid: np.ndarray, vocab: int, who: str = "") -> None:
    """``valid``: the ids that will be embedded (nn.Embedding raises on the same ones)"""
    if valid.size and (int(valid.min()) < 0 or int(valid.max()) >= vocab):
        raise IndexError(f"{who}token id out of range [0, {vocab}): min {int(valid.min())}, max {int(valid.max())} "
                         "(tokenizer / checkpoint mismatch?)")


def one_prompt(ids: np.ndarray, what: str) -> np.ndarray:
    """ONE prompt, [N] or [1, N], as [N]; ``what`` opens the refusal"""
    flat = ids[0] if ids.ndim == 2 and ids.shape[0] == 1 else ids
    if flat.ndim != 1:
        raise ValueError(f"{what} ([N] or [1, N]), got input_ids of shape {tuple(ids.shape)}")
    return flat


def check_pixels(px, who: str = "") -> int:
    """``px``: (shape, name of the dtype) of ``pixel_values``, [tiles, 3, S, S] in bf16 -> tiles"""
    shape, dtype = px
    if len(shape) != 4:
        raise ValueError(f"{who}wrong pixel_values size: {tuple(shape)}")
    if dtype != "torch.bfloat16":
        raise TypeError(f"{who}pixel_values must be bfloat16 like the model (got {dtype})")
    return int(shape[0])


def context_length(cols: np.ndarray, N: int, context_len, who: str = "") -> int:
    """How many tokens of an N-token prompt a context holds.  ``context_len`` None: the column after the last <IMG_CONTEXT> (``cols``)
    cut down to a multiple of 64, the attention kernels' key-tile rule (0 without one); else an int in [1, N - 1], not a bool."""
    if context_len is None:
        return (int(cols[-1]) + 1) // 64 * 64 if cols.size else 0
    if isinstance(context_len, bool) or not isinstance(context_len, (int, np.integer)) or not 1 <= context_len <= N - 1:
        raise ValueError(f"{who}context_len must be None or an int in [1, {N - 1}] (the prompt has {N} tokens), got {context_len!r}")
    return int(context_len)


def check_context_unmasked(am: Optional[np.ndarray], N: int, K: int, who: str = "") -> None:
    """every one of the K context columns is a valid token (``am``: the prompt's mask, any shape of N entries, or None)"""
    if am is None:
        return
    am = am.astype(bool).reshape(-1)
    if am.shape[0] != N:
        raise ValueError(f"{who}attention_mask of {am.shape[0]} columns, the prompt has {N}")
    if not am[:K].all():
        raise ValueError(f"{who}masked column {int(np.flatnonzero(~am[:K])[0])} inside the context ({K} tokens): "
                         "attention_mask must be set on every context column")


def pack_tails(seqs):
    """``trim_last_layer``: the rows from each sequence's first selected one on - all the last decoder layer needs QUERIES for
    (moe_reward.py:226-243).  ``seqs``, in packing order: (base, index of r, index of g, length, columns) - token i at packed row
    base + i and position columns[i].  -> tail_rows, tail_pos, cu_tail and, per sequence, the tail rows' indices of its r and g."""
    tail_rows, tail_pos, cu_tail, sel_r, sel_g = [], [], [0], [], []
    for base, lr, lg, L, cols in seqs:
        t0 = min(lr, lg)
        tb = cu_tail[-1] - t0
        tail_rows.append(base + np.arange(t0, L))
        tail_pos.append(cols[t0:])
        sel_r.append(tb + lr)
        sel_g.append(tb + lg)
        cu_tail.append(tb + L)
    return np.concatenate(tail_rows).astype(np.int32), np.concatenate(tail_pos).astype(np.int32), np.asarray(cu_tail, dtype=np.int32), sel_r, sel_g


class ReadoutRow(NamedTuple):
    """one selected row of a sample for the frame readout, in PACKED key coordinates (key i = the sample's i-th valid column)"""
    keys: int            # the keys the row sees: its own packed position + 1
    edges: np.ndarray    # int32 [bins + 1]: ascending, from 0 to ``keys``; bin b = keys [edges[b], edges[b + 1])
    fold: np.ndarray     # int32 [bins]: the public column each bin is summed into


class ReadoutBins(NamedTuple):
    n_frames: int        # F: public columns are frames 0 .. F - 1, then F = prompt text, F + 1 = caption
    reward: ReadoutRow
    gating: ReadoutRow


READOUT_MAX_BINS = 128   # bins per query of mjv_attention_readout_bf16


def readout_bins(rules: TokenRules, ids: np.ndarray, cols: np.ndarray, tiles_per_frame) -> ReadoutBins:
    """The frame readout's bins of ONE sample.  ``ids``: its [N] token ids; ``cols``: its valid columns in ascending order (the
    mask as ``analyse_ids`` packs it: right padding, left padding or holes alike); ``tiles_per_frame``: an int, or one int per
    frame.  The sample's <IMG_CONTEXT> tokens are dealt to the frames in column order, ``tiles_per_frame[f] * tokens_per_tile``
    each - frames may be separate runs with labels between them or one long run.  Every valid column carries a label: its frame
    for an image token, "prompt text" for any other token up to the last image token, "caption" behind it; a bin is a maximal run
    of packed keys with one label - text, frame 0, text, frame 1, ..., caption for a prompt with frame labels - so a bin is
    contiguous whatever the frames look like, and ``fold`` sums the bins of one label into its public column.  Per selected row
    (``selected_columns``) the bins are cut at the row's own position: a reward or gating row that sits before the last frame sees
    a partial bin and none behind it.  ``ValueError`` for a ``tiles_per_frame`` that does not account for the image tokens, image
    tokens or selected rows at masked columns, and more bins than a launch takes."""
    ids = np.asarray(ids)
    cols = np.asarray(cols, dtype=np.int64)
    N, tpt = ids.shape[0], rules.tokens_per_tile
    valid = np.zeros(N, dtype=bool)
    valid[cols] = True
    img = np.flatnonzero(ids == rules.ctx_id)
    if not valid[img].all():
        raise ValueError("frame readout: <IMG_CONTEXT> tokens in the masked part of the sequence")
    if isinstance(tiles_per_frame, (int, np.integer)) and not isinstance(tiles_per_frame, bool):
        per = int(tiles_per_frame) * tpt
        if per <= 0 or img.size == 0 or img.size % per:
            raise ValueError(f"frame readout: tiles_per_frame {int(tiles_per_frame)} x {tpt} image tokens per tile does not divide "
                             f"the prompt's {img.size} <IMG_CONTEXT> tokens")
        tiles = [int(tiles_per_frame)] * (img.size // per)
    else:
        tiles = [int(t) for t in tiles_per_frame]
        if not tiles or min(tiles) <= 0 or sum(tiles) * tpt != img.size:
            raise ValueError(f"frame readout: tiles_per_frame {tiles} x {tpt} image tokens per tile = {sum(tiles) * tpt}, the prompt "
                             f"holds {img.size} <IMG_CONTEXT> tokens")
    F = len(tiles)
    label = np.full(N, F, dtype=np.int32)                       # prompt text
    label[img] = np.repeat(np.arange(F, dtype=np.int32), np.asarray(tiles) * tpt)
    label[int(img[-1]) + 1:] = F + 1                            # caption
    lab = label[cols]                                           # per packed key
    starts = np.concatenate([[0], np.flatnonzero(lab[1:] != lab[:-1]) + 1]).astype(np.int32)   # first key of every bin
    loc = np.cumsum(valid) - 1
    r, g = selected_columns(ids, rules.pad_id, rules.gating_pattern)
    rows = []
    for what, c in (("reward", r), ("gating", g)):
        if not valid[c]:
            raise ValueError(f"frame readout: {what} row {c} lies in the masked part of the sequence")
        keys = int(loc[c]) + 1
        nb = int(np.searchsorted(starts, keys, "left"))         # bins that start before the row's last key
        if nb > READOUT_MAX_BINS:
            raise ValueError(f"frame readout: the {what} row sees {nb} runs of text / frame tokens, a launch takes {READOUT_MAX_BINS} bins")
        rows.append(ReadoutRow(keys, np.concatenate([starts[:nb], [keys]]).astype(np.int32), lab[starts[:nb]].astype(np.int32)))
    return ReadoutBins(F, rows[0], rows[1])


# ------------------------------------------------------------------------------------------------ the analysers
def analyse_ids(rules: TokenRules, ids: np.ndarray, am: Optional[np.ndarray], n_tiles: int, prefix_lookup=None):
    """Validates the batch and derives everything the kernels need from the token ids (packed ids, positions, row maps).
    ``prefix_lookup`` (``forward`` with ``prefix_cache`` on): called with the ids of the batch's common prompt prefix - the
    longest run of leading tokens shared by every sequence that ends before any <IMG_CONTEXT> / selected row, cut to a
    multiple of 64 - and returns True when the language tower's keys / values of exactly those tokens are cached: the
    packed rows then leave the first ``skip`` tokens of every sequence out (positions keep counting from 0)."""
    if ids.ndim != 2:
        raise ValueError(f"input_ids must be [batch, seq], got {ids.shape}")
    B, N = ids.shape
    if rules.pad_id is None and B != 1:
        raise ValueError("Cannot handle batch sizes > 1 if no padding token is defined.")
    if rules.ctx_id is None:
        raise ValueError("model.model.img_context_token_id is not set (eval_genai_mjvideo.py:115)")
    am = normalise_mask(am, ids.shape)
    # ANY mask.  The reference's eager path adds a [B, 1, N, N] mask of {causal, key is valid} (modeling_internlm2.py:96-125,907-913)
    # and numbers positions 0 .. N - 1 WITHOUT looking at the mask (:893-898): a valid query sees exactly the valid keys at or before
    # its column, rotated by their COLUMN indices.  Packing a row's valid tokens in column order, with those columns as positions,
    # is the same computation - right padding, left padding or holes alike; rows at masked columns are never read (checked below).
    lens = am.sum(axis=1)
    if (lens <= 0).any():
        raise ValueError("empty sequence in the batch")
    check_vocabulary(ids[am], rules.vocab)
    rs, gs, ctx, cols, loc = [], [], [], [], []
    for b in range(B):
        r, g = selected_columns(ids[b], rules.pad_id, rules.gating_pattern)
        if not am[b, r] or not am[b, g]:
            raise ValueError(f"sample {b}: reward row {r} / gating row {g} lies in the masked part of the sequence "
                             f"({int(lens[b])} valid tokens)")
        c = np.flatnonzero(ids[b] == rules.ctx_id)
        if not am[b, c].all():
            raise ValueError(f"sample {b}: <IMG_CONTEXT> tokens in the masked part of the sequence")
        rs.append(r)
        gs.append(g)
        ctx.append(c)
        cols.append(np.flatnonzero(am[b]))                   # valid columns, in order = the packed rows of this sample
        loc.append(np.cumsum(am[b]) - 1)                     # column -> index among the valid ones
    n_ctx = sum(c.size for c in ctx)
    if n_ctx != n_tiles * rules.tokens_per_tile:
        raise ValueError(f"{n_ctx} <IMG_CONTEXT> tokens in input_ids but pixel_values holds {n_tiles} tiles x {rules.tokens_per_tile} "
                         "image tokens (the reference would silently truncate, modeling_internvl_chat.py:178-186)")
    # the batch's common prompt prefix (system prompt + "Frame1: <img>": conversation.py:354-365, eval_genai_mjvideo.py:132-137)
    skip, prefix_ids = 0, None
    if prefix_lookup is not None:
        lim = min(min(int(c[0]) if c.size else N for c in ctx), min(rs), min(gs))
        masked = np.flatnonzero(~am[:, :lim].all(axis=0))     # (a prefix column must be a valid token of every sample)
        if masked.size:
            lim = int(masked[0])
        if B > 1 and lim > 0:
            differ = np.flatnonzero((ids[1:, :lim] != ids[0, :lim]).any(axis=0))
            if differ.size:
                lim = int(differ[0])
        cand = (lim // 64) * 64
        if cand > 0:
            prefix_ids = np.ascontiguousarray(ids[0, :cand])
            if prefix_lookup(prefix_ids):
                skip = cand
    packed, positions, img_rows, seqs, cu = [], [], [], [], [0]
    for b in range(B):
        L, lb = int(lens[b]), loc[b]
        base = cu[-1] - skip           # packed row of the token at column j of this sample = base + loc[j]  (j >= skip)
        packed.append(ids[b][cols[b][skip:]])
        positions.append(cols[b][skip:])
        img_rows.append(base + lb[ctx[b]])
        cu.append(base + L)
        seqs.append((base, lb[rs[b]], lb[gs[b]], L, cols[b]))
    tail_rows, tail_pos, cu_tail, sel_r, sel_g = pack_tails(seqs)
    return dict(B=B, N=N, total=cu[-1], max_len=int(lens.max()) - skip, skip=skip, prefix_ids=prefix_ids,
                ids=np.concatenate(packed).astype(np.int32), positions=np.concatenate(positions).astype(np.int32),
                cu=np.asarray(cu, dtype=np.int32), img_rows=np.concatenate(img_rows).astype(np.int32),
                sel_rows=np.asarray([s[0] + s[1] for s in seqs] + [s[0] + s[2] for s in seqs], dtype=np.int32),
                tail_rows=tail_rows, tail_pos=tail_pos, cu_tail=cu_tail, max_tail=int(np.diff(cu_tail).max()),
                sel_in_tail=np.asarray(sel_r + sel_g, dtype=np.int32))


def analyse_captions(rules: TokenRules, ids: np.ndarray, am: Optional[np.ndarray], ctxs, ci: np.ndarray, group: bool):
    """Validates every caption row against its context (nothing is repaired) and derives the packed own rows: what
    ``analyse_ids`` derives for whole prompts, for the columns behind each row's context.  ``group``: pack the sequences
    context by context (the "per-context" launches address a context's sequences as one range)."""
    M, N = ids.shape
    if rules.pad_id is None and M != 1:
        raise ValueError("Cannot handle batch sizes > 1 if no padding token is defined.")
    am = normalise_mask(am, ids.shape)
    check_vocabulary(ids[am], rules.vocab)
    toff = np.concatenate([[0], np.cumsum([c.tail_cols.size for c in ctxs])])
    sel, own_cols, img_src = [], [], []
    for b in range(M):
        row, c = ids[b], ctxs[int(ci[b])]
        P = c.P
        if N < P:
            raise ValueError(f"row {b}: {N} columns, its context {int(ci[b])} holds {P} tokens")
        differ = np.flatnonzero(row[:P] != c.ids)
        if differ.size:
            raise ValueError(f"row {b}: its first {P} token ids differ from those of its context {int(ci[b])} "
                             f"(first at column {int(differ[0])})")
        if not am[b, :P].all():
            raise ValueError(f"row {b}: masked column {int(np.flatnonzero(~am[b, :P])[0])} inside its context ({P} tokens)")
        r, g = selected_columns(row, rules.pad_id, rules.gating_pattern)
        if r < P or g < P:
            raise ValueError(f"row {b}: reward row {r} / gating row {g} lies inside its context ({P} tokens)")
        if not am[b, r] or not am[b, g]:
            raise ValueError(f"row {b}: reward row {r} / gating row {g} lies in the masked part of the sequence")
        ic = np.flatnonzero(row == rules.ctx_id)
        if ic.size != c.n_img:
            raise ValueError(f"row {b}: {ic.size} <IMG_CONTEXT> tokens, its context {int(ci[b])} was built from {c.n_img}")
        if not am[b, ic].all():
            raise ValueError(f"row {b}: <IMG_CONTEXT> tokens in the masked part of the sequence")
        cols = P + np.flatnonzero(am[b, P:])
        src = np.full(cols.shape[0], -1, dtype=np.int32)       # row of the contexts' image-tail table, or -1
        tail = ic[ic >= P]
        src[np.searchsorted(cols, tail)] = toff[int(ci[b])] + np.arange(tail.size)
        sel.append((int(np.searchsorted(cols, r)), int(np.searchsorted(cols, g))))     # r, g among the own rows
        own_cols.append(cols)
        img_src.append(src)
    order = np.argsort(ci, kind="stable") if group else np.arange(M)
    cu, seqs = [0], []
    for b in order:
        seqs.append((cu[-1], *sel[b], own_cols[b].shape[0], own_cols[b]))
        cu.append(cu[-1] + own_cols[b].shape[0])
    tail_rows, tail_pos, cu_tail, sel_r, sel_g = pack_tails(seqs)
    # the selected rows follow the ORIGINAL row order, whatever the packing order
    rows = np.zeros((4, M), dtype=np.int32)
    rows[:, order] = [[s[0] + s[1] for s in seqs], [s[0] + s[2] for s in seqs], sel_r, sel_g]
    return dict(M=M, N=N, total=cu[-1], order=order, index=ci[order].astype(np.int32),
                ids=np.concatenate([ids[b][own_cols[b]] for b in order]).astype(np.int32),
                positions=np.concatenate([own_cols[b] for b in order]).astype(np.int32),
                img_src=np.concatenate([img_src[b] for b in order]).astype(np.int32),
                cu=np.asarray(cu, dtype=np.int32), sel_rows=np.concatenate([rows[0], rows[1]]),
                tail_rows=tail_rows, tail_pos=tail_pos, cu_tail=cu_tail, sel_in_tail=np.concatenate([rows[2], rows[3]]))


def analyse_video(rules: TokenRules, px, ids: np.ndarray, am=None, who: str = "", context_len=None):
    """The checks of ``encode_video`` / ``encode_videos`` on ONE video and its prompt ([N] or [1, N]; nothing is repaired), and
    what the context pass needs of them: the first P ids, P (``context_length``), the <IMG_CONTEXT> columns and how many lie
    inside P.  ``who``: what the messages of a many-video call start with."""
    tiles = check_pixels(px, who)
    ids = one_prompt(ids, f"{who}ONE prompt per video")
    N = int(ids.shape[0])
    cols = np.flatnonzero(ids == rules.ctx_id)
    n_img = tiles * rules.tokens_per_tile
    if cols.size != n_img or n_img == 0:
        raise ValueError(f"{who}{cols.size} <IMG_CONTEXT> tokens in input_ids but pixel_values holds {tiles} tiles x "
                         f"{rules.tokens_per_tile} image tokens")
    P = context_length(cols, N, context_len, who)
    if P <= 0:
        raise ValueError(f"{who}the video tokens end at column {int(cols[-1])}: no multiple of 64 tokens to keep as a context")
    check_context_unmasked(am, N, P, who)
    check_vocabulary(ids[:P], rules.vocab, who)
    return dict(ids=ids[:P].copy(), N=N, P=P, tiles=tiles, n_img=n_img, n_in=int((cols < P).sum()), cols=cols)


def analyse_videos(rules: TokenRules, pxs, ids_list, masks=None, context_len=None):
    """``encode_videos``' checks - ``analyse_video`` video by video, every message naming its video - and the packed layout of
    the context pass.  ``pxs`` / ``ids_list`` (/ ``masks``): per video what ``analyse_video`` takes."""
    V = len(pxs)
    if not V:
        raise ValueError("encode_videos: empty list of videos")
    if len(ids_list) != V or (masks is not None and len(masks) != V):
        raise ValueError(f"encode_videos: {V} videos, {len(ids_list)} prompts" + ("" if masks is None else f", {len(masks)} attention masks"))
    if context_len is None or isinstance(context_len, (int, float, np.number)):   # one rule for every video
        lens = [context_len] * V
    else:
        lens = list(context_len)
        if len(lens) != V:
            raise ValueError(f"encode_videos: {V} videos, context_len of {len(lens)} entries (None, one int, or one per video)")
    vids = []
    for v in range(V):
        vids.append(analyse_video(rules, pxs[v], ids_list[v], None if masks is None else masks[v], f"video {v}: ", lens[v]))
        if pxs[v][0][1:] != pxs[0][0][1:]:
            raise ValueError(f"video {v}: tiles of {pxs[v][0][1:]}, video 0 has {pxs[0][0][1:]} (one vision-tower pass takes one tile size)")
    # the packed context rows (video v at rows cu[v] ...) and, behind them, every video's image tokens past its P
    cu = np.concatenate([[0], np.cumsum([x["P"] for x in vids])]).astype(np.int32)
    cu_tail = np.concatenate([[0], np.cumsum([x["n_img"] - x["n_in"] for x in vids])]).astype(np.int32)
    total = int(cu[-1])
    img_rows = np.concatenate([np.concatenate([cu[v] + x["cols"][:x["n_in"]], total + cu_tail[v] + np.arange(x["n_img"] - x["n_in"])])
                               for v, x in enumerate(vids)]).astype(np.int32)
    return dict(videos=vids, V=V, cu=cu, cu_tail=cu_tail, total=total, max_len=max(x["P"] for x in vids),
                N=max(x["N"] for x in vids), ids=np.concatenate([x["ids"] for x in vids]).astype(np.int32),
                positions=np.concatenate([np.arange(x["P"]) for x in vids]).astype(np.int32), img_rows=img_rows)


def analyse_extension(rules: TokenRules, ctx, ids: np.ndarray, px=None, am=None, context_len=None):
    """The checks of ``extend_context`` (nothing is repaired) and what its pass needs: the new context's length K, the ids of the new
    tokens [ctx.P, K), and for every new row the row of [parent's ``img_tail`` | new tiles' projections] that is spliced into it
    (-1: a text token).  ``px`` None: a text extension.  (``analyse_video``: the same steps from an empty parent.)"""
    tiles = 0 if px is None else check_pixels(px)
    if px is not None and not tiles:
        raise ValueError("pixel_values holds no tile: pass None for a pure text extension")
    ids = one_prompt(ids, "ONE prompt")
    N, P0 = int(ids.shape[0]), ctx.P
    if N <= P0:
        raise ValueError(f"the prompt has {N} tokens, the context to extend holds {P0}: nothing to add")
    differ = np.flatnonzero(ids[:P0] != ctx.ids)
    if differ.size:
        raise ValueError(f"the prompt's first {P0} token ids differ from those of the context to extend "
                         f"(first at column {int(differ[0])})")
    cols = np.flatnonzero(ids == rules.ctx_id)
    n_new = tiles * rules.tokens_per_tile
    if cols.size != ctx.n_img + n_new:
        raise ValueError(f"{cols.size} <IMG_CONTEXT> tokens in input_ids, but the context was built from {ctx.n_img} and "
                         f"pixel_values holds {tiles} new tiles x {rules.tokens_per_tile} image tokens")
    K = context_length(cols, N, context_len)
    if K <= P0:
        raise ValueError(f"the extended context would hold {K} tokens, the context to extend holds {P0} already: context_len must be greater")
    check_context_unmasked(am, N, K)
    check_vocabulary(ids[P0:K], rules.vocab)
    # image token j of the prompt (in column order) carries embedding j of the video: j < n_in0 lie inside the parent,
    # n_in0 <= j < ctx.n_img are the parent's img_tail, the rest the new tiles' tokens
    n_in0, n_in = ctx.n_img - int(ctx.tail_cols.size), int((cols < K).sum())
    if int((cols < P0).sum()) != n_in0:
        raise ValueError("the context to extend does not match its own image-token count")   # (cannot happen: ids agree)
    src = np.full(K - P0, -1, dtype=np.int32)
    src[cols[n_in0:n_in] - P0] = np.arange(n_in - n_in0)
    return dict(ids=ids[:K].copy(), new_ids=ids[P0:K].astype(np.int32), N=N, K=K, tiles=tiles, n_new=n_new, cols=cols,
                n_in0=n_in0, n_in=n_in, src=src)
