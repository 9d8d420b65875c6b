"""Many captions per video: ``encode_video`` + ``score_captions`` against ``forward`` on the same full prompts.

    python tools/caption_bench.py [--m 1,2,4,8,16,64] [--reps 5] [--out FILE.json] [--matrix 8x8] [--size 448] [--frames 8]
                                  [--context video,shared] [--no-forward] [--grow M]

MJ-VIDEO-2B dims, random-init weights generated on the device (bench.py's), 8 frames @448^2, captions of 24 - 96 tokens.
(``--m ""``: the matrix part alone.)  Per M: ms of ``encode_video``; ms of ``score_captions`` with caption_attention "shared" and "per-context" (alternated rep by rep
in this one process); ms of ``forward`` on the M full prompts in batches of at most 8 videos (all the model could do before:
the baseline); captions/s.  Every shape is warmed first; a timed region is bracketed by device events and ends in a
synchronise.  Then the library profiler's per-tag table of one caption pass (attention share, small-GEMM share) and V x M
through ``harness.score_caption_matrix`` - one video per ``encode_video`` call against all V through ONE ``encode_videos`` call,
and one ``score_captions`` call over the V contexts with ``caption_context_rows`` "packed" against "in-place" - the arms of
every pair alternated rep by rep.  ``--context video,shared`` adds the pair of context rules: a context that ends at the video
tokens cut down to a multiple of 64 (``encode_video``'s default) against one that holds the whole prefix the M prompts share
(``harness.shared_prefix_len``) - per M the context tokens, caption rows, ``score_captions`` ms and encode ms of both arms, and
the V x M matrix under ``context="video"`` / ``"shared"``, alternated rep by rep like every other pair.  ``--no-forward`` leaves
the ``forward`` baseline out.  ``--grow M`` adds the growth mode (``model.extend_context``): per added frame, one
``extend_context`` with that frame's tile against ``encode_video`` at the longer length; ``harness.score_growing_video`` over
lengths 1 .. frames under M captions against as many ``encode_video`` + ``score_captions`` rounds; and the bytes an instruction
branch adds against a cloned context - every pair alternated rep by rep.  One JSON document on stdout (and in --out).
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from mj_video_amd import configuration as C, harness, ops, synth  # noqa: E402
from mj_video_amd.chat_input import num_image_tokens_per_tile  # noqa: E402
from mj_video_amd.modeling import InternVLChatRewardModeling  # noqa: E402


class CharTokenizer:
    """duck-typed tokenizer for the harness call: the special tokens are single ids, every other character one id"""
    special = {"<|im_start|>": 92543, "<|im_end|>": 92542, "<img>": 92544, "</img>": 92545, "<IMG_CONTEXT>": 92546}

    def convert_tokens_to_ids(self, t):
        return self.special[t]

    def __call__(self, text, return_tensors="pt"):
        ids, i = [1], 0
        while i < len(text):
            for tok, tid in self.special.items():
                if text.startswith(tok, i):
                    ids.append(tid)
                    i += len(tok)
                    break
            else:
                if text.startswith("assistant", i):
                    ids += [525, 11353]
                    i += 9
                else:
                    ids.append(364 if text[i] == "\n" else 1000 + (ord(text[i]) % 50000))
                    i += 1
        t = torch.tensor([ids])
        return {"input_ids": t, "attention_mask": torch.ones_like(t)}


def timed(fn, reps):
    """median / min ms of ``fn`` over ``reps`` runs, device events around work that ends in a synchronise"""
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), reps=reps)


def alternated(arms, reps):
    """{name: fn} -> {name: median / min ms}: every arm warmed once, then the arms in turn, ``reps`` rounds"""
    for fn in arms.values():
        fn()
    ms = {name: [] for name in arms}
    for _ in range(reps):
        for name, fn in arms.items():
            ms[name].append(timed(fn, 1)["median_ms"])
    return {name: dict(median_ms=statistics.median(v), min_ms=min(v), reps=len(v), all_ms=[round(x, 3) for x in v])
            for name, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", default="1,2,4,8,16,64")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--size", type=int, default=448)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--matrix", default="8x8")
    ap.add_argument("--out", default=None)
    ap.add_argument("--context", default="video", help="video, or video,shared: the pair of context rules, alternated")
    ap.add_argument("--no-forward", action="store_true", help="leave the forward baseline out")
    ap.add_argument("--grow", type=int, default=0, help="growth mode under this many captions (0: off)")
    args = ap.parse_args()
    context_arms = [a for a in args.context.split(",") if a]
    if not context_arms or any(a not in ("video", "shared") for a in context_arms):
        ap.error("--context takes video, shared or both")
    dev = torch.device("cuda:0")
    cfg = C.InternVLChatRewardModelingConfig(**C.mjvideo_2b_config_dict(args.size), **C.mjvideo_head_kwargs())
    model = InternVLChatRewardModeling.from_config(cfg, dtype=torch.bfloat16, device=dev)
    bench.random_init_on_device(model, cfg, dev, seed=0)
    model.config.pad_token_id = synth.PAD_ID
    model.model.img_context_token_id = synth.IMG_CONTEXT_ID
    model.eval()
    n_img = args.frames * num_image_tokens_per_tile(cfg)
    px = synth.synth_pixel_values(7, 0, args.frames, args.size).to(dev)
    doc = dict(config=f"MJ-VIDEO-2B dims, {args.frames} frames @{args.size}^2, captions of 24 - 96 tokens", device=torch.cuda.get_device_name(0),
               rows=[])

    def prompts_of(M):
        return [synth.synth_input_ids(n_img, 900 + i, n_caption=24 + (i * 37) % 73) for i in range(M)]

    def forward_all(ids, mask, M):
        for lo in range(0, M, 8):
            hi = min(M, lo + 8)
            model.forward(px.repeat(hi - lo, 1, 1, 1), ids[lo:hi], mask[lo:hi])

    for M in [int(x) for x in args.m.split(",") if x]:
        prompts = prompts_of(M)
        ids, mask = synth.pad_batch(prompts)
        ids, mask = ids.to(dev), mask.to(dev)
        ctx = model.encode_video(px, prompts[0])
        for mode in ("shared", "per-context"):       # warm every shape
            model.caption_attention = mode
            model.score_captions(ctx, ids, mask)
        if not args.no_forward:
            forward_all(ids, mask, M)
        torch.cuda.synchronize()
        row = dict(M=M, context_tokens=ctx.P, context_bytes=ctx.nbytes, caption_rows=int(mask.sum().item()) - M * ctx.P)
        row["encode_video"] = timed(lambda: model.encode_video(px, prompts[0]), args.reps)
        res = {"shared": [], "per-context": []}
        for _ in range(args.reps):                    # the two versions alternated within one process
            for mode in ("shared", "per-context"):
                model.caption_attention = mode
                res[mode].append(timed(lambda: model.score_captions(ctx, ids, mask), 1)["median_ms"])
        for mode, ms in res.items():
            row[f"score_captions[{mode}]"] = dict(median_ms=statistics.median(ms), min_ms=min(ms), reps=len(ms))
        model.caption_attention = "shared"
        cap = row["score_captions[shared]"]["median_ms"]
        row["captions_per_s"] = dict(encode_plus_shared=1e3 * M / (row["encode_video"]["median_ms"] + cap), shared_warm_context=1e3 * M / cap)
        if not args.no_forward:
            row["forward"] = timed(lambda: forward_all(ids, mask, M), max(2, args.reps // 2))
            row["captions_per_s"]["forward"] = 1e3 * M / row["forward"]["median_ms"]
        if len(context_arms) > 1:   # the two context rules on the same prompts (caption_attention "shared")
            klen = {"video": None, "shared": harness.shared_prefix_len(prompts, synth.PAD_ID)}
            ctxs = {a: model.encode_video(px, prompts[0], context_len=klen[a]) for a in context_arms}
            enc = alternated({a: (lambda a=a: model.encode_video(px, prompts[0], context_len=klen[a])) for a in context_arms}, args.reps)
            sc = alternated({a: (lambda a=a: model.score_captions(ctxs[a], ids, mask)) for a in context_arms}, args.reps)
            row["context_arms"] = {a: dict(context_tokens=ctxs[a].P, caption_rows=int(mask.sum().item()) - M * ctxs[a].P,
                                           encode_video=enc[a], score_captions=sc[a]) for a in context_arms}
            print(f"M={M}: " + "; ".join(f"context {a}: {v['context_tokens']} tokens, {v['caption_rows']} caption rows, score_captions "
                                         f"{v['score_captions']['median_ms']:.2f} ms, encode {v['encode_video']['median_ms']:.2f} ms"
                                         for a, v in row["context_arms"].items()), file=sys.stderr, flush=True)
            del ctxs
        # the library profiler's per-tag table of ONE caption pass
        ops.prof_enable(True)
        ops.prof_reset()
        model.score_captions(ctx, ids, mask)
        tags = ops.prof_results()
        ops.prof_enable(False)
        ops.prof_reset()
        total = sum(t["ms"] for t in tags.values())
        row["caption_pass_tags"] = {k: dict(launches=t["launches"], ms=round(t["ms"], 4), share=round(t["ms"] / total, 4),
                                            tflops=round(t["flops"] / t["ms"] / 1e9, 2) if t["ms"] > 0 else 0.0)
                                    for k, t in sorted(tags.items(), key=lambda kv: -kv[1]["ms"])}
        row["caption_pass_shares"] = dict(attention=round(sum(t["ms"] for k, t in tags.items() if k.startswith("attn")) / total, 4),
                                          gemm=round(sum(t["ms"] for k, t in tags.items() if k.startswith("gemm")) / total, 4),
                                          sum_of_kernels_ms=round(total, 4))
        doc["rows"].append(row)
        print(f"M={M}: encode {row['encode_video']['median_ms']:.2f} ms, score_captions shared {cap:.2f} / per-context "
              f"{row['score_captions[per-context]']['median_ms']:.2f} ms" +
              ("" if args.no_forward else f", forward {row['forward']['median_ms']:.2f} ms"), file=sys.stderr, flush=True)
        del ctx

    if args.matrix:
        from mj_video_amd.chat_input import prepare_chat_input, video_prefix
        V, M = (int(x) for x in args.matrix.split("x"))
        tok = CharTokenizer()
        videos = [synth.synth_pixel_values(7, v, args.frames, args.size).to(dev) for v in range(V)]
        captions = ["".join(chr(97 + (i * 7 + j) % 26) for j in range(24 + (i * 37) % 73)) for i in range(M)]
        reps = max(2, args.reps)

        def matrix(per_call):
            return lambda: harness.score_caption_matrix(model, cfg, tok, videos, captions, {}, max_rows=64, videos_per_call=per_call)

        doc["matrix"] = dict(V=V, M=M, note="host tokenisation of the V x M prompts included; ceil(V M / 64) score_captions calls",
                             score_caption_matrix=alternated({"videos_per_call=1": matrix(1), f"videos_per_call={V}": matrix(V)}, reps))
        # the same call's parts on their own: the V encodes (one call per video / one call for all), and ONE score_captions
        # call of V * M rows over V contexts: contexts read in place / gathered into one packed buffer per layer / one launch per
        # context
        rows = [[prepare_chat_input(cfg, tok, pv, video_prefix(pv.shape[0]) + c, {}, device="cpu")[0] for c in captions] for pv in videos]
        ids, mask = harness.pad_right([r for per in rows for r in per], model.config.pad_token_id)
        ids, mask = ids.to(dev), mask.to(dev)
        index = torch.tensor([v for v in range(V) for _ in range(M)])
        firsts = [rows[v][0] for v in range(V)]
        doc["matrix"]["encode"] = alternated({"encode_video_x_V": lambda: [model.encode_video(pv, firsts[v]) for v, pv in enumerate(videos)],
                                              "encode_videos": lambda: model.encode_videos(videos, firsts)}, reps)

        def score(ctxs, rows_mode, attention):
            def run():
                model.caption_context_rows, model.caption_attention = rows_mode, attention
                model.score_captions(ctxs, ids, mask, context_index=index)
            return run

        owned = [model.encode_video(pv, firsts[v]) for v, pv in enumerate(videos)]
        views = model.encode_videos(videos, firsts)
        doc["matrix"]["context_bytes"] = dict(per_video=owned[0].nbytes, view_keeps_alive=views[0].storage_nbytes)
        doc["matrix"]["score_captions"] = alternated({"shared,packed": score(owned, "packed", "shared"),
                                                      "shared,in-place": score(owned, "in-place", "shared"),
                                                      "shared,in-place,views": score(views, "in-place", "shared"),
                                                      "per-context": score(owned, "in-place", "per-context")}, reps)
        model.caption_context_rows, model.caption_attention = "in-place", "shared"
        if len(context_arms) > 1:
            # the whole harness call under both context rules, and its parts: the V encodes and ONE score_captions call
            def matrix_ctx(a):
                return lambda: harness.score_caption_matrix(model, cfg, tok, videos, captions, {}, max_rows=64, context=a)

            klen = {"video": [None] * V, "shared": [harness.shared_prefix_len(rows[v], model.config.pad_token_id) for v in range(V)]}
            ctxs = {a: [model.encode_video(pv, firsts[v], context_len=klen[a][v]) for v, pv in enumerate(videos)] for a in context_arms}
            n_rows = int(mask.sum().item())
            doc["matrix"]["context_arms"] = dict(
                context_tokens={a: [c.P for c in ctxs[a]] for a in context_arms},
                caption_rows={a: n_rows - M * sum(c.P for c in ctxs[a]) for a in context_arms},
                score_caption_matrix=alternated({a: matrix_ctx(a) for a in context_arms}, reps),
                encode_video_x_V=alternated({a: (lambda a=a: [model.encode_video(pv, firsts[v], context_len=klen[a][v])
                                                              for v, pv in enumerate(videos)]) for a in context_arms}, reps),
                score_captions=alternated({a: score(ctxs[a], "in-place", "shared") for a in context_arms}, reps))
    if args.grow:
        from mj_video_amd.chat_input import prepare_chat_input, video_prefix
        M, F, per = args.grow, args.frames, num_image_tokens_per_tile(cfg)
        reps = max(2, args.reps)
        model.caption_context_rows, model.caption_attention = "in-place", "shared"
        end = lambda ids: int((ids[0] == synth.IMG_CONTEXT_ID).nonzero()[-1]) + 1  # noqa: E731  (the column behind the image run)
        firsts = [synth.synth_input_ids(n * per, 900, n_caption=24) for n in range(1, F + 1)]
        parents = [model.encode_video(px[:n], firsts[n - 1], context_len=end(firsts[n - 1])) for n in range(1, F)]
        steps = []
        for n in range(2, F + 1):   # n - 1 frames cached, frame n arrives
            ids_n, K = firsts[n - 1], end(firsts[n - 1])
            arms = alternated({"extend_context": lambda n=n: model.extend_context(parents[n - 2], ids_n, px[n - 1:n], context_len=K),
                               "encode_video": lambda n=n: model.encode_video(px[:n], ids_n, context_len=K)}, reps)
            steps.append(dict(frames=n, context_tokens=K, new_rows=K - parents[n - 2].P, **arms))
            print(f"grow to {n} frames: extend_context {arms['extend_context']['median_ms']:.2f} ms, encode_video "
                  f"{arms['encode_video']['median_ms']:.2f} ms", file=sys.stderr, flush=True)
        del parents
        tok = CharTokenizer()
        captions = ["".join(chr(97 + (i * 7 + j) % 26) for j in range(24 + (i * 37) % 73)) for i in range(M)]
        lengths = list(range(1, F + 1))

        def rounds():
            for n in lengths:
                rows = [prepare_chat_input(cfg, tok, px[:n], video_prefix(n) + c, {}, device="cpu")[0] for c in captions]
                ctx = model.encode_video(px[:n], rows[0], context_len=end(rows[0]))
                ids, mask = harness.pad_right(rows, model.config.pad_token_id)
                model.score_captions(ctx, ids.to(dev), mask.to(dev))

        growing = alternated({"score_growing_video": lambda: harness.score_growing_video(model, cfg, tok, px, captions, {}, lengths=lengths),
                              "encode_video+score_captions rounds": rounds}, reps)
        # one video under another instruction: what a branch adds against a copy of the context
        prompts = prompts_of(M)
        parent = model.encode_video(px, prompts[0])
        branch = model.extend_context(parent, prompts[0], context_len=harness.shared_prefix_len(prompts, synth.PAD_ID))
        doc["grow"] = dict(M=M, frames=F, per_added_frame=steps, lengths=lengths, growing=growing,
                           branch_bytes=dict(parent_tokens=parent.P, branch_tokens=branch.P, branch_adds=branch.nbytes,
                                             branch_keeps_alive=branch.storage_nbytes, cloned_context=branch.clone().nbytes),
                           note="host tokenisation of the prompts included in both growing arms")
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
