"""The token-layout analysis recorded case by case: one script for any two commits that must analyse prompts alike.

    python tools/layout_sweep.py --host [--out FILE.json]        no GPU: the five analysers and ``harness.shared_prefix_len``
    python tools/layout_sweep.py --gpu [--out FILE.json]         one MI355X: the public calls at tiny dims
    python tools/layout_sweep.py --time-ids [--calls 300]        no GPU: median wall time of ``_analyse_ids`` on bench.py's batch

Everything goes through ``model._analyse_ids`` / ``_analyse_captions`` / ``_analyse_video`` / ``_analyse_videos`` /
``_analyse_extension``, ``harness.shared_prefix_len`` and the public calls, so the same file runs on a commit and on its parent.

``--host``: a fixed seed, the tiny config, ids of ``mj_video_amd.synth``, contexts as CPU ``VideoContext`` objects without rows.
Every analyser gets valid inputs (right / left / holey masks, ``pad_id`` None and set, prefix lookup refused and accepted,
``group`` on and off, ``context_len`` None / inside the image run / at its end / behind it, parents with and without an
``img_tail``, text-only extensions) and inputs with one thing wrong.  Per case the record is every returned value - arrays as
(dtype, shape, SHA-256 of the bytes), scalars with their type - or the exception's type and message; printed: a SHA-256 over
all records and per analyser how many cases returned and raised.  Asserted here: at least 3 000 cases, at least half of every
analyser's cases return, and every refusal branch is seen (``REFUSALS``).  The message of the vocabulary refusal is recorded
up to ``token id out of range [0, V)``: what follows that differs between the analysers' wordings and carries no layout.

``--gpu``: ``forward`` (prefix cache off / on, last layer trimmed / whole), ``encode_video``, ``encode_videos`` of three videos,
``extend_context`` (a frame extension, a text-only branch), ``score_captions`` under both ``caption_attention`` settings and
over a segmented context - a hash of every output tensor's bytes and of every context's ``k`` / ``v`` / ``img_tail``, and the
launch census of the library's profiler (tag: launches, flops, bytes).
"""
import argparse
import hashlib
import json
import os
import re
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import mj_video_amd  # noqa: E402,F401
from mj_video_amd import configuration as C, harness, synth  # noqa: E402
from mj_video_amd.chat_input import num_image_tokens_per_tile  # noqa: E402
from mj_video_amd.modeling import InternVLChatRewardModeling, VideoContext  # noqa: E402

SIZE = 56                      # tile size of the tiny config: 4 image tokens per tile, the first <IMG_CONTEXT> at column 71
PAD, CTX = synth.PAD_ID, synth.IMG_CONTEXT_ID
CPU = torch.device("cpu")

# every refusal branch, as a pattern of its message (the analysers' own; "videos" also passes its videos' refusals through)
REFUSALS = {
    "ids": [r"input_ids must be \[batch, seq\]", r"Cannot handle batch sizes > 1", r"img_context_token_id is not set",
            r"attention_mask shape", r"empty sequence in the batch", r"token id out of range", r"Token pattern not found",
            r"lies in the masked part of the sequence", r"<IMG_CONTEXT> tokens in the masked part",
            r"<IMG_CONTEXT> tokens in input_ids but pixel_values holds"],
    "captions": [r"Cannot handle batch sizes > 1", r"attention_mask shape", r"token id out of range", r"columns, its context",
                 r"token ids differ from those of its context", r"masked column \d+ inside its context", r"Token pattern not found",
                 r"lies inside its context", r"lies in the masked part of the sequence", r"<IMG_CONTEXT> tokens, its context",
                 r"<IMG_CONTEXT> tokens in the masked part"],
    "video": [r"wrong pixel_values size", r"pixel_values must be bfloat16", r"ONE prompt per video",
              r"<IMG_CONTEXT> tokens in input_ids but pixel_values holds", r"no multiple of 64 tokens to keep",
              r"context_len must be None or an int", r"attention_mask of \d+ columns", r"masked column \d+ inside the context",
              r"token id out of range"],
    "videos": [r"SEQUENCES", r"empty list of videos", r"\d+ videos, \d+ prompts$", r"\d+ prompts, \d+ attention masks",
               r"context_len of \d+ entries", r"video \d+: tiles of", r"video \d+: wrong pixel_values size",
               r"video \d+: pixel_values must be bfloat16", r"video \d+: ONE prompt per video", r"video \d+: \d+ <IMG_CONTEXT> tokens",
               r"video \d+: the video tokens end", r"video \d+: context_len must be", r"video \d+: attention_mask of",
               r"video \d+: masked column", r"video \d+: token id out of range"],
    "extension": [r"first argument is the VideoContext", r"wrong pixel_values size", r"pixel_values must be bfloat16",
                  r"holds no tile", r"ONE prompt \(", r"nothing to add", r"differ from those of the context to extend",
                  r"but the context was built from", r"context_len must be None or an int", r"the extended context would hold",
                  r"attention_mask of \d+ columns", r"masked column \d+ inside the context", r"token id out of range",
                  r"does not match its own image-token count"],
    "shared_prefix_len": [r"needs at least one prompt", r"share no token", r"Token pattern not found"],
}


# ------------------------------------------------------------------------------------------------ recording
def digest(a: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


def canon(v):
    """a returned value as plain JSON: arrays as (dtype, shape, hash of the bytes), scalars with their type"""
    if isinstance(v, np.ndarray):
        return ["array", str(v.dtype), list(v.shape), digest(v)]
    if isinstance(v, dict):
        return {k: canon(v[k]) for k in sorted(v)}
    if isinstance(v, (list, tuple)):
        return [canon(x) for x in v]
    if v is None or isinstance(v, (bool, int, float, str, np.generic)):
        return [type(v).__name__, None if v is None else v.item() if isinstance(v, np.generic) else v]
    raise TypeError(f"unrecorded type {type(v)}")


class Recorder:
    def __init__(self):
        self.sha = hashlib.sha256()
        self.counts = {k: [0, 0] for k in REFUSALS}
        self.seen = {k: set() for k in REFUSALS}
        self.cases = 0

    def run(self, name: str, fn, *args, **kw):
        """one case: records what ``fn`` returns or raises; returns the value (None after a refusal)"""
        out = None
        try:
            out = fn(*args, **kw)
            rec = ["returned", canon(out)]
            self.counts[name][0] += 1
        except (ValueError, IndexError, TypeError) as e:
            msg = re.sub(r"(token id out of range \[0, \d+\)).*$", r"\1", str(e))
            rec = ["raised", type(e).__name__, msg]
            self.counts[name][1] += 1
            hit = [p for p in REFUSALS[name] if re.search(p, msg)]
            assert hit, f"{name}: a refusal that REFUSALS does not list: {type(e).__name__}: {msg}"
            self.seen[name].update(hit)
        self.sha.update(json.dumps([name, self.cases, rec], sort_keys=True).encode())
        self.cases += 1
        return out

    def summary(self) -> dict:
        for who, (ok, bad) in self.counts.items():
            assert 2 * ok >= ok + bad, f"{who}: {ok} of {ok + bad} cases return - the digest would mostly compare messages"
            missing = [p for p in REFUSALS[who] if p not in self.seen[who]]
            assert not missing, f"{who}: refusal branches never hit: {missing}"
        assert self.cases >= 3000, self.cases
        return dict(cases=self.cases, sha256=self.sha.hexdigest(),
                    returned_raised={k: dict(returned=a, raised=b) for k, (a, b) in self.counts.items()})


# ------------------------------------------------------------------------------------------------ inputs
def tiny_model():
    cfg = C.InternVLChatRewardModelingConfig(**C.tiny_config_dict(SIZE), **C.mjvideo_head_kwargs())
    model = InternVLChatRewardModeling.from_config(cfg, dtype=torch.bfloat16)
    model.config.pad_token_id = PAD
    model.model.img_context_token_id = CTX
    return cfg, model


def prompt(per, tiles, seed, n_caption, interleave=None):
    return synth.synth_input_ids(tiles * per, seed, n_caption=n_caption, interleave_frames=interleave)


def pixels(tiles, size=SIZE, dtype=torch.bfloat16):
    return torch.zeros(tiles, 3, size, size, dtype=dtype)


def fake_context(row: np.ndarray, P: int) -> VideoContext:
    """a context of the first ``P`` tokens of ``row`` without rows: all the analysers read of one"""
    cols = np.flatnonzero(row == CTX)
    return VideoContext(row[:P].copy(), P, [], [], torch.empty(int((cols >= P).sum()), 8), cols[cols >= P], int(cols.size), None,
                        None, None, CPU)


def pick(rng, seq):
    return seq[int(rng.integers(len(seq)))]


def holes(rng, mask: np.ndarray, ids: np.ndarray, lo: int = 0) -> np.ndarray:
    """masks a few plain text columns behind ``lo`` out of every row (never a special token, never the last five or the pad)"""
    mask = mask.copy()
    for b in range(ids.shape[0]):
        L = int(mask[b].sum())
        ok = [c for c in range(lo, L - 6) if 1000 <= ids[b, c] < 60000]
        for c in rng.choice(ok, size=min(len(ok), int(rng.integers(1, 4))), replace=False) if ok else []:
            mask[b, int(c)] = False
    return mask


def context_lens(rng, row: np.ndarray, shared: int):
    """``context_len`` values of every kind for one prompt: None, inside the image run, at its end, behind it"""
    cols = np.flatnonzero(row == CTX)
    first, end = int(cols[0]), int(cols[-1]) + 1
    return [None, int(rng.integers(1, first + 1)), int(rng.integers(first + 1, end)) if end > first + 1 else end, end,
            int(rng.integers(end, shared + 1)), shared, np.int64(end)]


BAD_LENS = (0, -1, 64.0, "64", True, "N")        # "N": the prompt's length


# ------------------------------------------------------------------------------------------------ the six sweeps
def sweep_ids(rec, model, per, rng, n):
    for case in range(n):
        B = int(rng.integers(1, 6))
        tiles = [int(rng.integers(1, 5)) for _ in range(B)]
        rows = [prompt(per, t, int(rng.integers(1 << 20)), int(rng.integers(1, 41)),
                       interleave=t if rng.random() < 0.15 else None) for t in tiles]
        if rng.random() < 0.3:            # the pairs of the evaluation: neighbours share their prompt
            rows = [rows[i - i % 2] for i in range(B)]
            tiles = [tiles[i - i % 2] for i in range(B)]
        ids_t, mask_t = synth.pad_batch(rows)
        mode = pick(rng, ["right", "right", "left", "holes", "none"])
        if mode == "left":
            ids_t, mask_t = synth.remask(ids_t, mask_t, "left")
        ids, am = ids_t.numpy().copy(), mask_t.numpy().astype(bool)
        if mode == "holes":
            am = holes(rng, am, ids)
        n_tiles = sum(tiles)
        model.config.pad_token_id, model.model.img_context_token_id = PAD, CTX
        lookup = pick(rng, [None, lambda p: True, lambda p: False, lambda p: bool(p.shape[0] > 64)])
        fault = pick(rng, [None] * 18 + ["ndim", "nopad", "noctx", "amshape", "empty", "vocab", "vocab_masked", "nopattern",
                                         "mask_sel", "mask_img", "tiles", "pad_in_caption"])
        am_arg = None if mode == "none" else am          # (no mask over a padded batch: the pads count as tokens)
        if fault is None and B == 1 and rng.random() < 0.5:
            model.config.pad_token_id = None
        if fault == "ndim":
            ids = ids[0] if rng.random() < 0.5 else ids[None]
        elif fault == "nopad":
            model.config.pad_token_id = None
        elif fault == "noctx":
            model.model.img_context_token_id = None
        elif fault == "amshape":
            am_arg = am[:, :-1] if rng.random() < 0.5 else am[:1].repeat(B + 1, axis=0)
        elif fault == "empty":
            am_arg = am.copy()
            am_arg[int(rng.integers(B))] = False
        elif fault in ("vocab", "vocab_masked"):
            b = int(rng.integers(B))
            c = int(rng.integers(2, 60)) if fault == "vocab" else ids.shape[1] - 1
            if fault == "vocab_masked":
                am_arg = am.copy()
                am_arg[b, c] = False        # (masked selected column: refused for that, not for the id)
            ids[b, c] = pick(rng, [-1, 92553, 1 << 40])
        elif fault == "nopattern":
            b = int(rng.integers(B))
            ids[b][ids[b] == synth.GATING_PATTERN[2]] = 1234
        elif fault == "mask_sel":
            b = int(rng.integers(B))
            L = int(np.flatnonzero(am[b])[-1])
            am_arg = am.copy()
            am_arg[b, L - int(rng.integers(0, 5))] = False
        elif fault == "mask_img":
            b = int(rng.integers(B))
            am_arg = am.copy()
            am_arg[b, int(pick(rng, np.flatnonzero(ids[b] == CTX)))] = False
        elif fault == "tiles":
            n_tiles += pick(rng, [-1, 1])
        elif fault == "pad_in_caption" and mode in ("right", "holes"):     # the reward row is the token before the FIRST pad
            b = int(rng.integers(B))
            ids[b, int(np.flatnonzero(am[b])[-1]) - 7] = PAD
        rec.run("ids", model._analyse_ids, ids, am_arg, n_tiles, lookup)
    model.config.pad_token_id, model.model.img_context_token_id = PAD, CTX


def caption_family(per, rng, tiles, m):
    """``m`` full prompts of one video: the same video tokens, captions of their own"""
    seed = int(rng.integers(1 << 20))
    return [prompt(per, tiles, seed + j, int(rng.integers(1, 41))) for j in range(m)]


def sweep_captions(rec, model, per, rng, n):
    for case in range(n):
        V = int(rng.integers(1, 4))
        tiles = [int(rng.integers(1, 9)) for _ in range(V)]
        fams = [caption_family(per, rng, t, int(rng.integers(1, 4))) for t in tiles]
        prompts = [p for f in fams for p in f]
        ci = np.asarray([v for v, f in enumerate(fams) for _ in f], dtype=np.int64)
        order = rng.permutation(len(prompts))
        prompts, ci = [prompts[i] for i in order], ci[order]
        M = len(prompts)
        ctxs = []
        for f in fams:
            shared = harness.shared_prefix_len(f, PAD)
            ctxs.append(fake_context(f[0][0].numpy(), int(pick(rng, context_lens(rng, f[0][0].numpy(), shared)[1:] + [64, 64]))))
        ids_t, mask_t = synth.pad_batch(prompts)
        ids, am = ids_t.numpy().copy(), mask_t.numpy().astype(bool)
        if rng.random() < 0.3:
            am = holes(rng, am, ids, lo=max(c.P for c in ctxs))
        group = bool(rng.random() < 0.5)
        model.config.pad_token_id = PAD
        am_arg = am
        fault = pick(rng, [None] * 16 + ["nopad", "amshape", "vocab", "short", "differ", "mask_ctx", "nopattern", "inside",
                                         "mask_sel", "count", "mask_img"])
        if fault is None and M == 1 and rng.random() < 0.5:
            model.config.pad_token_id, am_arg = None, pick(rng, [None, am])
        b = int(rng.integers(M))
        P = ctxs[int(ci[b])].P
        if fault == "nopad":
            model.config.pad_token_id = None
        elif fault == "amshape":
            am_arg = am[:, :-1]
        elif fault == "vocab":
            ids[b, min(P + 1, ids.shape[1] - 6)] = pick(rng, [-5, 92553])
        elif fault == "short":
            longer = prompt(per, 8, 7, 60)[0].numpy()
            ctxs[int(ci[b])] = fake_context(longer, ids.shape[1] + int(rng.integers(1, 4))) if longer.shape[0] > ids.shape[1] + 4 else ctxs[int(ci[b])]
        elif fault == "differ":
            ids[b, int(rng.integers(P))] += 1
        elif fault == "mask_ctx":
            am_arg = am.copy()
            am_arg[b, int(rng.integers(P))] = False
        elif fault == "nopattern":
            ids[b][ids[b] == synth.GATING_PATTERN[2]] = 1234
        elif fault == "inside" and P > 8:      # a row that ends inside its context: pads behind P, the pattern in front of it
            ids[b, P:] = PAD
            ids[b, P - 6:P - 1] = synth.GATING_PATTERN
            am_arg = am.copy()
            am_arg[b, P:] = False
            ctxs[int(ci[b])] = fake_context(ids[b].copy(), P)
            ctxs[int(ci[b])].n_img = int((prompts[b][0].numpy() == CTX).sum())
            for o in range(M):
                if o != b and ci[o] == ci[b]:
                    ids[o, :P] = ids[b, :P]
        elif fault == "mask_sel":
            am_arg = am.copy()
            am_arg[b, int(np.flatnonzero(am[b])[-1]) - int(rng.integers(0, 5))] = False
        elif fault == "count":
            ctxs[int(ci[b])].n_img += pick(rng, [-1, 4])
        elif fault == "mask_img":
            tail = np.flatnonzero(ids[b] == CTX)
            tail = tail[tail >= P]
            if tail.size:
                am_arg = am.copy()
                am_arg[b, int(pick(rng, tail))] = False
        rec.run("captions", model._analyse_captions, ids, am_arg, ctxs, ci, group)
    model.config.pad_token_id = PAD


def video_case(per, rng, who):
    """one video and its prompt with (mostly) nothing wrong -> (pixels, ids tensor, mask or None, context_len, fault done)"""
    tiles = int(rng.integers(1, 9))
    fam = caption_family(per, rng, tiles, int(rng.integers(1, 4)))
    ids_t = fam[0]
    row = ids_t[0].numpy()
    N = row.shape[0]
    shared = harness.shared_prefix_len(fam, PAD)
    K = pick(rng, context_lens(rng, row, shared))
    P = int(K) if K is not None else 64
    px = pixels(tiles)
    am = pick(rng, [None, None, torch.ones(N, dtype=torch.bool), torch.ones(1, N, dtype=torch.long)])
    if am is not None and P + 1 < N and rng.random() < 0.4:
        am = am.clone()
        am.view(-1)[int(rng.integers(P, N))] = 0          # a hole behind the context: fine
    if rng.random() < 0.3:
        ids_t = ids_t[0]                                   # [N] instead of [1, N]
    fault = pick(rng, [None] * 18 + ["pxdim", "pxdtype", "two", "tiles", "noimg", "early", "len", "amlen", "mask_ctx", "vocab",
                                     "vocab_behind"])
    if fault == "pxdim":
        px = px[0]
    elif fault == "pxdtype":
        px = px.float()
    elif fault == "two":
        ids_t = ids_t.reshape(1, -1).repeat(2, 1)
    elif fault == "tiles":
        px = pixels(tiles + pick(rng, [-1, 1]))
    elif fault == "noimg":
        px, ids_t = pixels(0), prompt(per, 0, 3, 8)
    elif fault == "early":        # the video tokens end before column 64: no multiple of 64 to keep (default rule only)
        short = prompt(per, 1, 5, 8)[0]
        ids_t, px, K, am = torch.cat([short[:10], short[40:]])[None], pixels(1), None, None
    elif fault == "len":
        K = pick(rng, BAD_LENS)
        K = N if K == "N" else K
    elif fault == "amlen":
        am = torch.ones(N + pick(rng, [-1, 2]), dtype=torch.bool)
    elif fault == "mask_ctx":
        am = torch.ones(N, dtype=torch.bool)
        am[int(rng.integers(P))] = False
    elif fault in ("vocab", "vocab_behind"):
        ids_t = ids_t.clone()
        ids_t.view(-1)[int(rng.integers(1, P)) if fault == "vocab" and P > 1 else 0 if fault == "vocab" else N - 1] = pick(rng, [-1, 92553])
    return px, ids_t, am, K


def sweep_video(rec, model, per, rng, n):
    for case in range(n):
        px, ids_t, am, K = video_case(per, rng, "video")
        if rng.random() < 0.5:
            rec.run("video", model._analyse_video, px, ids_t, am, context_len=K)
        else:
            rec.run("video", model._analyse_video, px, ids_t, am, who=f"video {case % 7}: ", context_len=K)


def sweep_videos(rec, model, per, rng, n):
    for case in range(n):
        V = int(rng.integers(1, 5))
        clean = rng.random() < 0.8
        vids = []
        while len(vids) < V:
            v = video_case(per, rng, "videos")
            if clean:         # keep only videos the one-video analysis takes
                try:
                    model._analyse_video(v[0], v[1], v[2], context_len=v[3])
                except (ValueError, IndexError, TypeError):
                    continue
            vids.append(v)
        px, ids, masks, lens = ([v[i] for v in vids] for i in range(4))
        masks = None if all(m is None for m in masks) else masks
        how = pick(rng, ["each", "each", "none", "one"])
        if how == "none" and clean:
            lens = None
        elif how == "one" and clean:
            lens = int(rng.integers(1, 70))
        fault = pick(rng, [None] * 20 + ["tensor", "empty", "prompts", "masks", "lens", "tilesize", "float"])
        if fault == "tensor":
            px, ids = (px[0], ids[0]) if rng.random() < 0.5 else (px, ids[0])
        elif fault == "empty":
            px, ids, masks, lens = [], [], None, None
        elif fault == "prompts":
            ids = ids + [ids[0]] if rng.random() < 0.5 else ids[:-1]
        elif fault == "masks":
            masks = [torch.ones_like(ids[0])] * (V + 1)
        elif fault == "lens":
            lens = [64] * (V + 1)
        elif fault == "tilesize" and V > 1:
            px = list(px)
            px[V - 1] = px[V - 1][:, :, :28] if px[V - 1].dim() == 4 else px[V - 1]
        elif fault == "float":
            lens = 64.0
        rec.run("videos", model._analyse_videos, px, ids, masks, lens)


def sweep_extension(rec, model, per, rng, n):
    for case in range(n):
        text_only = rng.random() < 0.45
        t0 = int(rng.integers(1, 5))
        t1 = t0 if text_only else t0 + int(rng.integers(1, 5))
        seed = int(rng.integers(1 << 20))
        fam = [prompt(per, t1, seed + j, int(rng.integers(1, 41))) for j in range(int(rng.integers(1, 4)))]
        full = fam[0]
        row = full[0].numpy()
        N = row.shape[0]
        shared = harness.shared_prefix_len(fam, PAD)
        first = int(np.flatnonzero(row == CTX)[0])
        # the parent: a context of the first t0 tiles' prompt; its ids must be the full prompt's, so a frame extension's parent
        # ends inside its own image run at the latest (with an ``img_tail`` when it ends before the run's end)
        old = prompt(per, t0, seed, 4)[0].numpy()
        if text_only:
            P0 = int(pick(rng, [64, int(rng.integers(1, shared)), first + per * t0, int(rng.integers(first, first + per * t0 + 1))]))
            P0 = min(P0, shared - 1)
            old = row
        else:
            P0 = int(pick(rng, [64, int(rng.integers(1, first + per * t0 + 1)), first + per * t0]))
        parent = fake_context(old, P0)
        px = None if text_only else pixels(t1 - t0)
        lens = [k for k in context_lens(rng, row, shared) if (P0 < 64 if k is None else k > P0)] + [N - 1, int(rng.integers(P0 + 1, N))]
        K = pick(rng, lens)
        Kv = 64 if K is None else int(K)
        am = pick(rng, [None, None, torch.ones(N, dtype=torch.bool), torch.ones(1, N, dtype=torch.long)])
        if am is not None and Kv + 1 < N and rng.random() < 0.4:
            am = am.clone()
            am.view(-1)[int(rng.integers(Kv, N))] = 0
        ids_t = full[0] if rng.random() < 0.3 else full
        fault = pick(rng, [None] * 24 + ["ctx", "pxdim", "pxdtype", "notile", "two", "short", "differ", "count", "len", "notmore",
                                         "amlen", "mask_ctx", "vocab", "vocab_old", "own_count"])
        if fault == "ctx":
            parent = pick(rng, [None, row])
        elif fault == "pxdim":
            px = pixels(1)[0]
        elif fault == "pxdtype":
            px = pixels(max(t1 - t0, 1)).float()
        elif fault == "notile":
            px = pixels(0)
        elif fault == "two":
            ids_t = full.repeat(2, 1)
        elif fault == "short":
            ids_t = full[:, :P0 - int(rng.integers(0, 2))] if P0 > 1 else full[:, :1]
        elif fault == "differ":
            ids_t = full.clone()
            ids_t[0, int(rng.integers(P0))] += 1
        elif fault == "count":
            px = pixels(t1 - t0 + 1) if px is not None or rng.random() < 0.5 else None
            if px is None:
                parent.n_img += 4
        elif fault == "len":
            K = pick(rng, BAD_LENS)
            K = N if K == "N" else K
        elif fault == "notmore":
            K = int(rng.integers(1, P0 + 1))
        elif fault == "amlen":
            am = torch.ones(N + pick(rng, [-1, 2]), dtype=torch.bool)
        elif fault == "mask_ctx":
            am = torch.ones(N, dtype=torch.bool)
            am[int(rng.integers(Kv))] = False
        elif fault == "vocab":
            ids_t = full.clone()
            ids_t[0, int(rng.integers(P0, max(Kv, P0 + 1)))] = pick(rng, [-1, 92553])
        elif fault == "vocab_old":
            ids_t = full.clone()
            ids_t[0, N - 1] = 92553
        elif fault == "own_count":     # a context that contradicts itself (a real one cannot: its ids are the prompt's)
            parent.tail_cols = np.concatenate([parent.tail_cols, [N]]) if rng.random() < 0.5 or not parent.tail_cols.size else parent.tail_cols[:-1]
        rec.run("extension", model._analyse_extension, parent, ids_t, px, am, K)


def sweep_shared_prefix(rec, model, per, rng, n):
    for case in range(n):
        fam = caption_family(per, rng, int(rng.integers(1, 9)), int(rng.integers(1, 6)))
        if rng.random() < 0.3:
            fam.append(fam[int(rng.integers(len(fam)))])
        rows = list(fam)
        pad = pick(rng, [PAD, PAD, None])
        pattern = None
        how = pick(rng, ["plain", "padded", "numpy", "flat"])
        if how == "padded":
            rows = list(synth.pad_batch(fam)[0])
        elif how == "numpy":
            rows = [r.numpy() for r in fam]
        elif how == "flat":
            rows = [r[0] for r in fam]
        fault = pick(rng, [None] * 10 + ["empty", "nothing", "nopattern", "pattern", "pad_first"])
        if fault == "empty":
            rows = []
        elif fault == "nothing":
            rows = [r.clone() if isinstance(r, torch.Tensor) else r.copy() for r in rows] + [rows[0].clone() if isinstance(rows[0], torch.Tensor) else rows[0].copy()]
            rows[-1].reshape(-1)[0] += 1
        elif fault == "nopattern":
            pattern = (5, 6, 7)
        elif fault == "pattern":        # another tokenizer's marker: here the two ids that open every prompt's last turn
            pattern = synth.GATING_PATTERN[1:3]
        elif fault == "pad_first" and how == "padded" and pad is not None:
            rows = [r.clone() for r in rows]
            rows[0][0] = PAD            # a pad at column 0: the reward column wraps to the last one, as in the model
        rec.run("shared_prefix_len", harness.shared_prefix_len, rows, pad, pattern)


def host(out):
    cfg, model = tiny_model()
    per = num_image_tokens_per_tile(cfg)
    rec = Recorder()
    rng = np.random.Generator(np.random.Philox(key=[2024, 36]))
    sweep_ids(rec, model, per, rng, 900)
    sweep_captions(rec, model, per, rng, 800)
    sweep_video(rec, model, per, rng, 700)
    sweep_videos(rec, model, per, rng, 600)
    sweep_extension(rec, model, per, rng, 800)
    sweep_shared_prefix(rec, model, per, rng, 400)
    return dict(host=rec.summary())


# ------------------------------------------------------------------------------------------------ GPU
def tensor_hash(t: torch.Tensor) -> str:
    return hashlib.sha256(t.detach().contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()[:16]


FIELDS = ("rewards", "hidden_state", "prompt_embedding", "criteria_gating_output", "aspect_gating_output", "aspect_weights",
          "score", "weighted_scores", "aspect_scores")


def gpu(out):
    from mj_video_amd import ops
    dev = torch.device("cuda:0")
    cfg, _ = tiny_model()
    per = num_image_tokens_per_tile(cfg)
    model = InternVLChatRewardModeling.from_config(cfg, dtype=torch.bfloat16)
    model.load_state_dict(synth.synth_state_dict(cfg, seed=21), strict=True)
    model.config.pad_token_id = PAD
    model = model.to(torch.bfloat16).to(dev).eval()
    model.model.img_context_token_id = CTX
    hashes = {}

    def outputs(name, o):
        hashes[name] = {f: tensor_hash(getattr(o, f)) for f in FIELDS}
        hashes[name]["packed34"] = tensor_hash(model.last_packed34)

    def context(name, c):
        hashes[name] = dict(P=c.P, segments=[n for _, _, n in c.segments], k=[tensor_hash(t) for t in c.k],
                            v=[tensor_hash(t) for t in c.v], img_tail=tensor_hash(c.img_tail), tail_cols=c.tail_cols.tolist())

    ops.prof_reset()
    ops.prof_enable(True)
    tiles = (4, 3, 2)
    videos = [synth.synth_pixel_values(9, v, t, SIZE).to(dev) for v, t in enumerate(tiles)]
    caps = [[prompt(per, t, 100 * v + j, L) for j, L in enumerate((5, 17, 40))] for v, t in enumerate(tiles)]
    # forward: three videos under one caption each, a holey mask; prefix cache off / on (cold, then warm), last layer trimmed / whole
    ids_t, mask_t = synth.pad_batch([c[2] for c in caps])
    ids_t, mask_t = synth.remask(ids_t, mask_t, "holes")
    px = torch.cat(videos)
    for cache in (False, True):
        for trim in (True, False):
            model.prefix_cache, model.trim_last_layer = cache, trim
            for rep in range(2 if cache else 1):
                outputs(f"forward cache={cache} trim={trim} rep={rep}", model.forward(px, ids_t.to(dev), mask_t.to(dev)))
    model.prefix_cache, model.trim_last_layer = True, True
    # contexts: one video alone, three in one call, a frame extension of a two-tile context, a text-only branch
    shared = [harness.shared_prefix_len(c, PAD) for c in caps]
    one = model.encode_video(videos[0], caps[0][0])
    context("encode_video", one)
    many = model.encode_videos(videos, [c[0] for c in caps], context_len=[None, shared[1], 75])
    for v, c in enumerate(many):
        context(f"encode_videos[{v}]", c)
    half = model.encode_video(videos[0][:2], prompt(per, 2, 100, 5))
    grown = model.extend_context(half, caps[0][0], videos[0][2:], context_len=80)
    context("extend_context frames", grown)
    branch = model.extend_context(grown, caps[0][0], context_len=shared[0])
    context("extend_context text", branch)
    # captions: the three videos' nine prompts over the contexts of the one call; video 0's over the segmented context
    rows = [p for c in caps for p in c]
    ids_c, mask_c = (t.to(dev) for t in synth.pad_batch(rows))
    index = torch.tensor([v for v in range(3) for _ in range(3)])
    for how in ("shared", "per-context"):
        model.caption_attention = how
        ctxs = many if how == "shared" else model.encode_videos(videos, [c[0] for c in caps])
        outputs(f"score_captions {how}", model.score_captions(ctxs, ids_c, mask_c, context_index=index))
    model.caption_attention = "shared"
    ids_0, mask_0 = (t.to(dev) for t in synth.pad_batch(caps[0]))
    outputs("score_captions segmented", model.score_captions(branch, ids_0, mask_0))
    torch.cuda.synchronize()
    census = {tag: [r["launches"], r["flops"], r["bytes"]] for tag, r in sorted(ops.prof_results().items())}
    ops.prof_enable(False)
    sha = hashlib.sha256(json.dumps([hashes, census], sort_keys=True).encode()).hexdigest()
    return dict(gpu=dict(sha256=sha, hashes=hashes, launch_census_launches_flops_bytes=census))


# ------------------------------------------------------------------------------------------------ host time of _analyse_ids
def time_ids(calls: int):
    """median wall time of ``model._analyse_ids`` on the ids of bench.py's default batch (4 pairs of 8 tiles @448^2)"""
    cfg = C.InternVLChatRewardModelingConfig(**C.mjvideo_2b_config_dict(448), **C.mjvideo_head_kwargs())
    model = InternVLChatRewardModeling.from_config(cfg, dtype=torch.bfloat16, device="meta")
    model.config.pad_token_id = PAD
    model.model.img_context_token_id = CTX
    per = num_image_tokens_per_tile(cfg)
    rows = []
    for p in range(4):
        row = synth.synth_input_ids(per * 8, caption_seed=p)
        rows += [row, row]
    ids_t, mask_t = synth.pad_batch(rows)
    ids, am = ids_t.numpy(), mask_t.numpy().astype(bool)
    medians, fastest = [], []
    for rep in range(3):
        for _ in range(50):
            model._analyse_ids(ids, am, 64, lambda p: True)
        t = []
        for _ in range(calls):
            t0 = time.perf_counter()
            model._analyse_ids(ids, am, 64, lambda p: True)
            t.append(time.perf_counter() - t0)
        medians.append(round(1e6 * statistics.median(t), 2))
        fastest.append(round(1e6 * min(t), 2))
    return dict(analyse_ids_host_us=dict(calls=calls, warmup=50, medians_of_three_measurements=medians,
                                         median=statistics.median(medians), spread=round(max(medians) - min(medians), 2),
                                         fastest_call_of_each_measurement=fastest))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--gpu", action="store_true")
    ap.add_argument("--time-ids", action="store_true")
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    doc = {}
    if args.host:
        doc.update(host(args.out))
    if args.gpu:
        doc.update(gpu(args.out))
    if args.time_ids:
        doc.update(time_ids(args.calls))
    text = json.dumps(doc, indent=1, sort_keys=True)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
