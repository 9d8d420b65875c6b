"""Pairwise-preference evaluation protocol of the reference's only reward-model driver.

Follows scripts/eval/eval_genai_mjvideo.py:118-165: the same caption scored against the left and the right
video (two independent forwards), right wins iff ``score_right > score_left``, a video is "good" iff its score
is > 0, a tie vote is correct iff both are good, a both-bad vote iff both are bad; ``prefer_Acc`` counts only
left/right votes, ``Acc`` all four vote types.  The scoring itself is batched (and data-parallel through
mj_video_amd.parallel) instead of the reference's batch-1 Python loop.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Iterable, List, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .layout import selected_columns
from .chat_input import prepare_chat_input, video_prefix

VOTE_TYPES = ("leftvote", "rightvote", "bothbad_vote", "tievote")


@dataclass
class PreferenceCounts:
    prefer_truth: int = 0
    prefer_total: int = 0
    truth: int = 0
    total: int = 0

    def update(self, vote_type: str, score_left: float, score_right: float) -> None:
        left_good, right_good = score_left > 0, score_right > 0
        if vote_type == "rightvote":
            self.prefer_total += 1
            self.total += 1
            if score_right > score_left:
                self.prefer_truth += 1
                self.truth += 1
        elif vote_type == "leftvote":
            self.prefer_total += 1
            self.total += 1
            if score_right < score_left:
                self.prefer_truth += 1
                self.truth += 1
        elif vote_type == "bothbad_vote":
            self.total += 1
            if not left_good and not right_good:
                self.truth += 1
        elif vote_type == "tievote":
            self.total += 1
            if left_good and right_good:
                self.truth += 1

    @property
    def prefer_acc(self) -> float:
        return self.prefer_truth / self.prefer_total if self.prefer_total else float("nan")

    @property
    def acc(self) -> float:
        return self.truth / self.total if self.total else float("nan")


def evaluate_votes(votes: Iterable[Tuple[str, float, float]]) -> PreferenceCounts:
    c = PreferenceCounts()
    for vote_type, sl, sr in votes:
        c.update(vote_type, float(sl), float(sr))
    return c


def pad_right(ids_list: Sequence[torch.Tensor], pad_id: int):
    n = max(int(t.shape[-1]) for t in ids_list)
    ids = torch.full((len(ids_list), n), pad_id, dtype=torch.long)
    mask = torch.zeros((len(ids_list), n), dtype=torch.long)
    for i, t in enumerate(ids_list):
        k = int(t.shape[-1])
        ids[i, :k] = t.reshape(-1).cpu()
        mask[i, :k] = 1
    return ids, mask


def prefetch_to_device(batches: Iterable, device, depth: int = 1):
    """Yields the items of ``batches`` (tensors, or tuples / lists / dicts of tensors; anything else passes through) moved to
    ``device``, with the upload of the NEXT ``depth`` items already running on a copy stream of its own: batch i + 1 crosses
    PCIe while batch i is scored, so a caller that starts from host memory sees the HBM-resident rate (without this the copies
    sit on the scoring stream: -1.8 % with bf16 pixel tensors, -4.5 % with uint8 720p frames, profiles/r03_f_pcie_inclusive.txt).
    Host tensors are pinned here if they are not yet (an unpinned source makes the copy synchronous).  The yielded tensors are
    safe to use on the current stream (it waits for the copy's event; ``record_stream`` keeps the allocator from recycling
    them under the scoring kernels)."""
    from collections import deque
    device = torch.device(device)
    side = torch.cuda.Stream(device=device)

    def move(x, fn):
        if isinstance(x, torch.Tensor):
            return fn(x)
        if isinstance(x, dict):
            return {k: move(v, fn) for k, v in x.items()}
        if isinstance(x, (list, tuple)):
            return type(x)(move(v, fn) for v in x)
        return x

    def start(item):
        def up(t):
            if t.is_cuda:
                return t
            return (t if t.is_pinned() else t.pin_memory()).to(device, non_blocking=True)
        with torch.cuda.stream(side):
            dev_item = move(item, up)
            ev = torch.cuda.Event()
            ev.record(side)
        return dev_item, ev

    def finish(entry):
        dev_item, ev = entry
        cur = torch.cuda.current_stream(device)
        cur.wait_event(ev)
        move(dev_item, lambda t: (t.record_stream(cur), t)[1] if t.is_cuda else t)
        return dev_item

    pending = deque()
    for item in batches:
        pending.append(start(item))
        if len(pending) > depth:
            yield finish(pending.popleft())
    while pending:
        yield finish(pending.popleft())


@torch.no_grad()
def score_pair_batch(model, config, tokenizer, examples: Sequence[dict], generation_config: dict) -> torch.Tensor:
    """examples: dicts with ``prompt``, ``left_pixels``, ``right_pixels`` (each [F,3,S,S] bf16).  Both videos of
    every pair go through ONE packed forward; returns ``[len(examples), 2, 1 + n_aspects + n_objectives]`` fp32."""
    _lib.assert_product_library()   # an evaluation never scores on a diagnostics build of the kernels
    dev = model.model.device
    px, ids = [], []
    for ex in examples:
        for key in ("left_pixels", "right_pixels"):
            pv = ex[key].to(torch.bfloat16)
            q = video_prefix(pv.shape[0]) + ex["prompt"]
            i, _ = prepare_chat_input(config, tokenizer, pv, q, generation_config, device="cpu")
            px.append(pv)
            ids.append(i)
    pad_id = model.config.pad_token_id
    if pad_id is None:
        raise ValueError("model.config.pad_token_id must be set to batch pairs (eval_genai_mjvideo.py:112)")
    ids_b, mask = pad_right(ids, pad_id)
    model.forward(torch.cat(px).to(dev), ids_b.to(dev), mask.to(dev))
    return model.last_packed34.view(len(examples), 2, -1)


@torch.no_grad()
def score_with_frame_readout(model, config, tokenizer, pixels: torch.Tensor, caption: str, generation_config: dict,
                             tiles_per_frame=1):
    """ONE video ([tiles, 3, S, S]) under ONE caption, scored with the frame readout on: returns ``(CustomOutput, FrameReadout)`` -
    the scores ``model.forward`` gives with the readout off, bit for bit, and where the reward row and the gating row put their
    attention per decoder layer and head (``FrameReadout.per_frame()``: [1, frames]).  ``tiles_per_frame``: an int, or one int
    per frame (dynamic tiling: the tiles of one frame are summed into its column).  The model's ``frame_readout`` /
    ``readout_tiles_per_frame`` are restored afterwards."""
    _lib.assert_product_library()
    dev = model.model.device
    pv = pixels.to(torch.bfloat16)
    ids, mask = prepare_chat_input(config, tokenizer, pv, video_prefix(pv.shape[0]) + caption, generation_config, device="cpu")
    before = model.frame_readout, model.readout_tiles_per_frame
    model.frame_readout, model.readout_tiles_per_frame = True, tiles_per_frame
    try:
        out = model.forward(pv.to(dev), ids.to(dev), mask.to(dev))
        return out, model.last_readout
    finally:
        model.frame_readout, model.readout_tiles_per_frame = before


def shared_prefix_len(rows, pad_id, gating_pattern=None) -> int:
    """The longest context the full prompts ``rows`` of ONE video can share (``model.encode_video(..., context_len=...)``): the
    length of their common prefix, capped so that every row keeps its reward row r and its gating row g outside the context -
    min over rows of min(r, g), r and g as ``model.score_captions`` finds them (the last token before the first ``pad_id``;
    the last occurrence of the gating pattern).  ``rows``: 1-D id sequences ([N] or [1, N] tensors / arrays), padded or not.
    Two identical prompts share everything; the cap is what keeps their selected rows among the own rows."""
    rows = [np.asarray(r.detach().cpu() if isinstance(r, torch.Tensor) else r).reshape(-1) for r in rows]
    if not rows:
        raise ValueError("shared_prefix_len needs at least one prompt")
    n = min(r.shape[0] for r in rows)
    common = n
    for r in rows[1:]:
        differ = np.flatnonzero(r[:n] != rows[0][:n])
        if differ.size:
            common = min(common, int(differ[0]))
    cap = n
    for r in rows:
        cap = min(cap, *selected_columns(r, pad_id, gating_pattern))
    k = min(common, cap)
    if k < 1:
        raise ValueError("shared_prefix_len: the prompts share no token that every row can leave to a context")
    return k


@torch.no_grad()
def score_video_captions(model, config, tokenizer, pixels: torch.Tensor, captions: Sequence[str], generation_config: dict,
                         context: str = "video") -> torch.Tensor:
    """ONE video ([F, 3, S, S]) under M captions: the video goes through the vision tower and the context part of the
    language tower once (``model.encode_video``), every caption as its own rows only (``model.score_captions``).
    Returns ``[M, 1 + n_aspects + n_objectives]`` fp32 - the rows ``model.forward`` gives for the M full prompts, up to fp32
    summation order.  ``context``: as in ``score_caption_matrix``."""
    return score_caption_matrix(model, config, tokenizer, [pixels], captions, generation_config, context=context)[0]


@torch.no_grad()
def score_caption_matrix(model, config, tokenizer, videos: Sequence[torch.Tensor], captions: Sequence[str], generation_config: dict,
                         max_rows: int = 64, videos_per_call: int = 1, context: str = "video") -> torch.Tensor:
    """V videos x M captions (caption-vs-distractor matrices, perturbed captions, re-caption choice): every video is encoded
    once, the V * M caption rows go through ``model.score_captions`` in as few calls as ``max_rows`` rows per call allow.
    ``videos_per_call`` > 1: the videos go through ``model.encode_videos`` in blocks of that many (one vision-tower and one
    context pass per block), a block's rows are scored and its contexts dropped before the next block is encoded - the contexts
    alive at any time are one block's, whatever V is.  ``context``: "video" - a context ends at the video tokens, cut down to a
    multiple of 64 (``encode_video``'s default); "shared" - it holds the whole prefix the video's M prompts share
    (``shared_prefix_len``: the rest of the video, the frame labels, any instruction before the caption), so those rows are not
    recomputed per caption.  Returns ``[V, M, 1 + n_aspects + n_objectives]`` fp32."""
    _lib.assert_product_library()
    if max_rows < 1:
        raise ValueError("max_rows must be positive")
    if videos_per_call < 1:
        raise ValueError("videos_per_call must be positive")
    if context not in ("video", "shared"):
        raise ValueError(f"context {context!r} not in ('video', 'shared')")
    dev = model.model.device
    pad_id = model.config.pad_token_id
    if pad_id is None:
        raise ValueError("model.config.pad_token_id must be set to batch captions (eval_genai_mjvideo.py:112)")
    V, M = len(videos), len(captions)
    if not V or not M:
        raise ValueError("score_caption_matrix needs at least one video and one caption")

    def prompts_of(pv):
        return [prepare_chat_input(config, tokenizer, pv, video_prefix(pv.shape[0]) + c, generation_config, device="cpu")[0] for c in captions]

    def context_len_of(rows):
        if context == "video":
            return None
        return shared_prefix_len(rows, pad_id, getattr(model.config, "gating_token_pattern", None))

    def score_rows(ids, contexts, out):
        """rows r = video-major over ``contexts``; appends the packed rows of every call to ``out``"""
        n = len(ids)
        for lo in range(0, n, max_rows):
            hi = min(n, lo + max_rows)
            v0, v1 = lo // M, (hi - 1) // M
            ids_b, mask = pad_right(ids[lo:hi], pad_id)
            index = torch.tensor([r // M - v0 for r in range(lo, hi)], dtype=torch.int64)
            model.score_captions(contexts[v0:v1 + 1], ids_b.to(dev), mask.to(dev), context_index=index)
            out.append(model.last_packed34)

    out = []
    if videos_per_call == 1:
        ids, contexts = [], []
        for pv in videos:
            pv = pv.to(torch.bfloat16)
            rows = prompts_of(pv)
            ids.extend(rows)
            contexts.append(model.encode_video(pv.to(dev), rows[0], context_len=context_len_of(rows)))
        score_rows(ids, contexts, out)
    else:
        for b0 in range(0, V, videos_per_call):
            block = [pv.to(torch.bfloat16) for pv in videos[b0:b0 + videos_per_call]]
            rows = [prompts_of(pv) for pv in block]
            contexts = model.encode_videos([pv.to(dev) for pv in block], [r[0] for r in rows],
                                           context_len=None if context == "video" else [context_len_of(r) for r in rows])
            score_rows([r for per in rows for r in per], contexts, out)
            del contexts
    return torch.cat(out).view(V, M, -1)


@torch.no_grad()
def score_growing_video(model, config, tokenizer, pixels: torch.Tensor, captions: Sequence[str], generation_config: dict,
                        lengths: Sequence[int] = (2, 4, 8)) -> torch.Tensor:
    """ONE video ([F, 3, S, S], a tile per frame) scored under M captions at several lengths - its first ``lengths[0]`` frames,
    its first ``lengths[1]`` ... (ascending, <= F): dense / temporal reward, a clip that is still being generated.  The first
    length is encoded (``model.encode_video``), every further one EXTENDS the context before it (``model.extend_context``): the
    vision tower and the context pass run over each frame once, whatever the number of lengths, and no cached row is copied.
    The prompt of L frames is ``video_prefix(L) + caption`` - its image tokens are one run, so the prompt of a shorter length
    is a prefix of the longer one's up to the end of its own image run, and that column is where each context ends
    (``context_len``; ``caption_attention`` "shared" scores contexts of any length and segmented ones).
    Returns ``[len(lengths), M, 1 + n_aspects + n_objectives]`` fp32: row [i, j] = what ``model.forward`` gives for the first
    ``lengths[i]`` frames under caption j, up to fp32 summation order."""
    _lib.assert_product_library()
    dev = model.model.device
    pad_id = model.config.pad_token_id
    if pad_id is None:
        raise ValueError("model.config.pad_token_id must be set to batch captions (eval_genai_mjvideo.py:112)")
    lengths = [int(n) for n in lengths]
    if not lengths or not captions:
        raise ValueError("score_growing_video needs at least one length and one caption")
    if lengths[0] < 1 or any(b <= a for a, b in zip(lengths, lengths[1:])) or lengths[-1] > int(pixels.shape[0]):
        raise ValueError(f"lengths {lengths} must ascend strictly within [1, {int(pixels.shape[0])}] (the video's frames)")
    ctx_id = model.model.img_context_token_id
    pixels = pixels.to(torch.bfloat16)
    out, ctx, done = [], None, 0
    for n in lengths:
        pv = pixels[:n]
        rows = [prepare_chat_input(config, tokenizer, pv, video_prefix(n) + c, generation_config, device="cpu")[0] for c in captions]
        end = int(np.flatnonzero(rows[0].reshape(-1).numpy() == ctx_id)[-1]) + 1
        if ctx is None:
            ctx = model.encode_video(pv.to(dev), rows[0], context_len=end)
        else:
            ctx = model.extend_context(ctx, rows[0], pixels[done:n].to(dev), context_len=end)
        done = n
        ids_b, mask = pad_right(rows, pad_id)
        model.score_captions(ctx, ids_b.to(dev), mask.to(dev))
        out.append(model.last_packed34)
    return torch.stack(out)


# ---------------------------------------------------------------------------------------------------------------
# Collator batch format and MJ-BENCH-VIDEO label schema
@torch.no_grad()
def score_collated_batch(model, batch: dict):
    """Scores one batch in the training collator's layout (scripts/data_processor/dataset.py:445-554 as consumed by
    scripts/train/overall_train.py:70-82): ``video_{0,1}_pixel_values [B, F, 3, H, W]``, right-padded
    ``video_{0,1}_input_ids [B, N]`` and ``video_{0,1}_attention_mask``.  The 5-D pixel block is flattened to
    ``[B*F, 3, H, W]`` exactly as the trainer does; both videos of every pair go through one packed forward.
    Returns ``(output_video_0, output_video_1)`` (CustomOutput each)."""
    _lib.assert_product_library()
    dev = model.model.device
    outs = []
    px = [batch[f"video_{i}_pixel_values"] for i in (0, 1)]
    b, f, c, h, w = px[0].shape
    flat = torch.cat([p.reshape(-1, c, h, w) for p in px]).to(torch.bfloat16).to(dev)
    ids = [batch[f"video_{i}_input_ids"] for i in (0, 1)]
    n = max(int(t.shape[1]) for t in ids)
    pad = model.config.pad_token_id
    if pad is None:
        raise ValueError("model.config.pad_token_id must be set for collated batches (dataset.py pads with it)")

    def widen(t, fill):
        if t.shape[1] == n:
            return t
        extra = torch.full((t.shape[0], n - t.shape[1]), fill, dtype=t.dtype, device=t.device)
        return torch.cat([t, extra], dim=1)

    ids_all = torch.cat([widen(t, pad) for t in ids])
    mask_all = torch.cat([widen(batch[f"video_{i}_attention_mask"], 0) for i in (0, 1)])
    out = model.forward(flat, ids_all.to(dev), mask_all.to(dev))
    from .modeling import CustomOutput
    from dataclasses import fields
    for i in (0, 1):
        sl = slice(i * b, (i + 1) * b)
        outs.append(CustomOutput(**{fl.name: getattr(out, fl.name)[sl] for fl in fields(CustomOutput)}))
    return outs[0], outs[1]


def criteria_targets(labels: dict, mse: bool = True):
    """MJ-BENCH-VIDEO per-criterion labels -> (score, relevance, names): 1 = good -> (+1, relevant), 2 = bad ->
    (-1 with ``mse`` else 0, relevant), anything else -> (0, irrelevant)   (dataset.py:52-85)."""
    score, related, names = [], [], []
    for key, value in labels.items():
        names.append(key)
        score.append(1 if value == 1 else ((-1 if mse else 0) if value == 2 else 0))
        related.append(1 if value in (1, 2) else 0)
    return score, related, names


def overall_target(value, mse: bool = True):
    """Same mapping for a single overall label (dataset.py:57-69)."""
    return ([1], [1]) if value == 1 else (([-1 if mse else 0], [1]) if value == 2 else ([0], [0]))


def preference_targets(labels):
    """"Video 1 better" -> (0, counted), "Video 2 better" -> (1, counted), anything else -> (1, masked out)
    (dataset.py:87-112); ``labels`` is a dict of per-aspect strings or a single overall string."""
    values = list(labels.values()) if isinstance(labels, dict) else [labels]
    pref = [0 if v == "Video 1 better" else 1 for v in values]
    mask = [1 if v in ("Video 1 better", "Video 2 better") else 0 for v in values]
    return pref, mask


# ------------------------------------------------------------------------------------ MJ-BENCH-VIDEO (datas/test.json)
ASPECT_KEYS = ("Alignment", "Safety", "Fineness", "Consistency", "Bias")   # order of video_*_overall_score in test.json


@dataclass
class ConfusionCounts:
    """Per-dimension bookkeeping of scripts/train/overall_train.py:308-324 (``calculate_metrics``): predictions are the signs
    of the model's outputs (``> 0``), a label counts as positive when it EQUALS 1 and as negative when it EQUALS 0 (the
    dataset's default labels use -1 for "bad", dataset.py:52-85, which is neither - the reference's own quirk, reproduced),
    and only dimensions with a non-zero relevance mask are counted."""
    dims: int
    correct: np.ndarray = None
    total: np.ndarray = None
    tp: np.ndarray = None
    fp: np.ndarray = None
    tn: np.ndarray = None
    fn: np.ndarray = None

    def __post_init__(self):
        for f in ("correct", "total", "tp", "fp", "tn", "fn"):
            setattr(self, f, np.zeros(self.dims, dtype=np.float64))

    def update(self, predictions, ground_truth, mask) -> None:
        pred = np.asarray(predictions, dtype=bool).ravel()
        gt = np.asarray(ground_truth).ravel()
        active = np.asarray(mask).ravel() != 0
        self.correct += (pred.astype(gt.dtype) == gt) & active
        self.tp += pred & (gt == 1) & active
        self.fp += pred & (gt == 0) & active
        self.tn += ~pred & (gt == 0) & active
        self.fn += ~pred & (gt == 1) & active
        self.total += active

    def summary(self) -> dict:
        """The figures ``save_metrics`` reports (overall_train.py:326-388): pooled accuracy / precision / recall / F1 and the
        per-dimension vectors (a dimension that never occurs divides 0 by 0: NaN, as in the reference's tensors)."""
        def ratio(a, b):
            return float(a) / float(b) if b > 0 else 0
        tp, fp, tn, fn = self.tp, self.fp, self.tn, self.fn
        acc = ratio(self.correct.sum(), self.total.sum())
        rec = ratio(tp.sum(), (tp + fn).sum())
        pre = ratio(tp.sum(), (tp + fp).sum())
        f1 = 2 * (rec * pre) / (rec + pre) if (rec + pre) > 0 else 0
        with np.errstate(divide="ignore", invalid="ignore"):
            acc_d, rec_d, pre_d = self.correct / self.total, tp / (tp + fn), tp / (tp + fp)
            f1_d = 2 * (rec_d * pre_d) / (rec_d + pre_d)
        return dict(accuracy=acc, precision=pre, recall=rec, f1=f1, accuracy_dim=acc_d.tolist(), precision_dim=pre_d.tolist(),
                    recall_dim=rec_d.tolist(), f1_dim=f1_d.tolist(), tp=tp.tolist(), fp=fp.tolist(), tn=tn.tolist(), fn=fn.tolist())


def mjbench_targets(item: dict, mse: bool = True) -> dict:
    """Label tensors of one datas/test.json pair exactly as VideoDataset builds them (dataset.py:329-398): per video the
    criteria / aspect scores and relevance masks, plus the overall preference (0 = video 1 better, 1 = video 2 better) and
    its mask.  The two videos must carry the same label names (dataset.py:346,352)."""
    out = {}
    names = None
    for v in (0, 1):
        cs, cr, cn = criteria_targets(item[f"video_{v}_label"], mse=mse)
        a_s, a_r, an = criteria_targets(item[f"video_{v}_overall_score"], mse=mse)
        if names is not None and names != (cn, an):
            raise ValueError("the two videos of a pair carry different label names")
        names = (cn, an)
        out[f"video_{v}"] = dict(criteria_score=cs, criteria_related=cr, aspect_score=a_s, aspect_related=a_r)
    pref, mask = preference_targets(item["overall_preference"])
    out["overall_preference"], out["overall_mask"] = pref[0], mask[0]
    out["criteria_names"], out["aspect_names"] = names
    return out


def evaluate_mjbench(items: Sequence[dict], scores: "np.ndarray", mse: bool = True) -> dict:
    """MJ-BENCH-VIDEO evaluation of ``scores`` [pairs, 2, 1 + n_aspects + n_criteria] (the packed block of
    ``CustomOutput``: score, aspect_scores, rewards per video - what ``parallel.score_pairs_dp`` gathers) against the
    labels of ``items``: the overall preference accuracy of ``CustomTrainer.evaluate`` (overall_train.py:390-442:
    prefer_predict = not (score_0 > score_1), counted where the pair has a decisive overall preference) and the aspect /
    criteria sign metrics of ``evaluate_aspect`` (overall_train.py:204-306)."""
    scores = np.asarray(scores, dtype=np.float64)
    n_asp = len(items[0]["video_0_overall_score"])
    n_crit = len(items[0]["video_0_label"])
    assert scores.shape == (len(items), 2, 1 + n_asp + n_crit), scores.shape
    aspect, criteria = ConfusionCounts(n_asp), ConfusionCounts(n_crit)
    correct = count = 0
    for i, item in enumerate(items):
        t = mjbench_targets(item, mse=mse)
        for v in (0, 1):
            tv = t[f"video_{v}"]
            aspect.update(scores[i, v, 1:1 + n_asp] > 0, tv["aspect_score"], tv["aspect_related"])
            criteria.update(scores[i, v, 1 + n_asp:] > 0, tv["criteria_score"], tv["criteria_related"])
        prefer_predict = int(not (scores[i, 0, 0] > scores[i, 1, 0]))
        correct += int(prefer_predict == t["overall_preference"]) * t["overall_mask"]
        count += t["overall_mask"]
    return dict(overall_accuracy=(correct / count if count > 0 else 0), overall_correct=correct, overall_count=count,
                aspect=aspect.summary(), criteria=criteria.summary(), aspect_names=list(items[0]["video_0_overall_score"]),
                criteria_names=list(items[0]["video_0_label"]))
