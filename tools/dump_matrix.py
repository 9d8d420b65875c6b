"""Bit-for-bit record of what the scoring paths compute and launch, to compare two trees (a refactor against its parent).

    python tools/dump_matrix.py --out DIR [--cases PREFIX,PREFIX...]     # runs the cases with the tree this file sits in
    python tools/dump_matrix.py --compare DIR_A DIR_B                    # exit 1 + one line per difference

Per case a directory: every CustomOutput field and ``last_packed34``, the cached prefix rows / VideoContext tensors / probes the
case has, as raw .npy (bf16 viewed as int16: bits are compared), and prof.json = launches and flops per kernel name.  The
forward is deterministic (no atomics): two runs of one tree are identical.  Each case's GPU work runs once.  Cases:
  fwd_*       2B dims @224^2, the five videos of test_prefix_cache_is_invisible_and_invalidates: a cold and a warm forward
              under every entry of SETTINGS
  llm_layer   run_llm_layer(0, x) at tiny dims, x from a fixed seed
  phi3_*      the tiny Phi-3 tower and inputs of test_phi3_trimming_and_prefix_cache_are_invisible: prefix_cache x
              trim_last_layer, and "mxfp8"
  captions_*  tests/captions_util.py at tiny dims: the contexts of encode_video, score_captions under caption_attention x trim
"""
import argparse
import copy
import json
import os
import sys
from functools import partial

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

DEFAULTS = dict(prefix_cache=True, trim_last_layer=True, attention_scores="flash", norm_fusion=False, use_gemm_workspace=True,
                _exp_fp8_attn_side=False, debug_probes=None, caption_attention="shared")
SETTINGS = {"default": {}, "prefix_off": dict(prefix_cache=False), "trim_off": dict(trim_last_layer=False),
            "eager": dict(attention_scores="eager"), "norm_fusion": dict(norm_fusion=True), "no_ws": dict(use_gemm_workspace=False),
            "mxfp8": dict(fmt="mxfp8"), "mxfp8_rank999": dict(fmt="mxfp8-rank999"),
            "fp8_attn_side": dict(fmt="mxfp8", _exp_fp8_attn_side=True), "probes": dict(debug_probes={})}


def configure(model, fmt="bf16", **over):
    """every switch at its default except ``over``; nothing cached from the case before"""
    for k, v in {**DEFAULTS, **copy.deepcopy(over)}.items():
        setattr(model, k, v)
    model.set_ffn_format(fmt)
    model._prefix, model._prefix_misses, model._prefix_last_miss = None, 0, None
    return model


def save(d, name, t, model=None):
    """``t``: a tensor, a dict of them, or (with ``model``) a CustomOutput + the model's ``last_packed34``"""
    if model is not None:
        from util import FIELDS
        t = dict({f: getattr(t, f) for f in FIELDS}, last_packed34=model.last_packed34)
    if isinstance(t, dict):
        for k, v in t.items():
            save(d, f"{name}.{k}", v)
    elif isinstance(t, torch.Tensor):
        t = t.detach().contiguous().cpu()
        np.save(os.path.join(d, name + ".npy"), (t.view(torch.int16) if t.dtype == torch.bfloat16 else t).numpy())


def cold_and_warm(d, model, inputs):
    """a forward that meets no cached prefix and the one after it; a case with the cache on is void unless the second was served"""
    for tag in ("cold", "warm"):
        hits = model.prefix_cache_hits
        save(d, tag, model.forward(*inputs), model)
    if model.prefix_cache and model.debug_probes is None:
        assert model.prefix_cache_hits == hits + 1 and model._prefix["P"] == 64, "void case: the warm forward met no cached prefix"
        save(d, "prefix", {k: dict(enumerate(v)) if isinstance(v, list) else v for k, v in model._prefix.items() if k in ("k", "v", "v_last")})
    save(d, "probe", model.debug_probes or {})


def cases(dev):
    """-> (name, function(directory)) per case; the models are built when the first case that needs them runs"""
    import captions_util
    from util import build_hip_model, case_inputs, make_cfg
    from mj_video_amd import configuration as C, synth
    from mj_video_amd.chat_input import num_image_tokens_per_tile
    models = {}

    def model_of(kind):
        if kind not in models:
            if kind == "phi3":
                cd = C.tiny_phi3_config_dict(56)
                cd["llm_config"].update(hidden_size=384, num_attention_heads=4, num_key_value_heads=4, original_max_position_embeddings=160)
                cfg = C.InternVLChatRewardModelingConfig(**cd, **C.mjvideo_head_kwargs())
                models[kind] = build_hip_model(cfg, synth.synth_state_dict(cfg, seed=51), dev)
                models[kind].config.pad_token_id = synth.PHI3_TOKENS.pad
                models[kind].model.img_context_token_id = synth.PHI3_TOKENS.img_context
            else:
                cfg = make_cfg(kind, 224 if kind == "2b" else 56)
                sd = synth.synth_state_dict(cfg, seed=0, lm_head=False)
                sd["model.language_model.output.weight"] = torch.zeros(1, dtype=torch.bfloat16).expand(
                    cfg.llm_config.vocab_size, cfg.llm_config.hidden_size)
                models[kind] = build_hip_model(cfg, sd, dev)
        return models[kind]

    def fwd(over, d):
        model = configure(model_of("2b"), **over)
        vids = [dict(video_idx=i, n_tiles=t, caption_seed=i) for i, t in enumerate([8, 6, 8, 3, 5])]
        cold_and_warm(d, model, [t.to(dev) for t in case_inputs(model.config, vids, 77, 224)[:3]])

    def llm_layer(d):
        model = configure(model_of("tiny"))
        x = synth._normal(7, "dump_matrix/llm_layer", (2, 70, model.config.llm_config.hidden_size), 1.0).to(torch.bfloat16)
        save(d, "out", model.run_llm_layer(0, x))

    def phi3(over, d):
        model = configure(model_of("phi3"), **over)
        per, tk = num_image_tokens_per_tile(model.config), synth.PHI3_TOKENS
        ids, mask = synth.pad_batch([synth.synth_input_ids(per * t, i, tokens=tk) for i, t in enumerate([4, 2, 3])], pad_id=tk.pad)
        px = torch.cat([synth.synth_pixel_values(300, i, t, 56) for i, t in enumerate([4, 2, 3])])
        cold_and_warm(d, model, [px.to(dev), ids.to(dev), mask.to(dev)])

    def captions(case, d):
        model = configure(model_of("tiny"))
        _, videos, prompts, index = captions_util.CASES[case]("tiny")
        ids, mask = (t.to(dev) for t in synth.pad_batch(prompts))
        ctxs = [model.encode_video(v.to(dev), prompts[int(np.flatnonzero(index == i)[0])]) for i, v in enumerate(videos)]
        save(d, "ctx", {i: dict(enumerate(c.tensors())) for i, c in enumerate(ctxs)})
        for mode in ("shared", "per-context"):
            for trim in (True, False):
                model.caption_attention, model.trim_last_layer = mode, trim
                save(d, f"{mode}.trim{int(trim)}", model.score_captions(ctxs, ids, mask, context_index=torch.from_numpy(index)), model)

    yield from ((f"fwd_{name}", partial(fwd, over)) for name, over in SETTINGS.items())
    yield "llm_layer", llm_layer
    for name, over in (("cache1_trim1", {}), ("cache0_trim1", dict(prefix_cache=False)), ("cache1_trim0", dict(trim_last_layer=False)),
                       ("cache0_trim0", dict(prefix_cache=False, trim_last_layer=False)), ("mxfp8", dict(fmt="mxfp8"))):
        yield f"phi3_{name}", partial(phi3, over)
    yield from ((f"captions_{case}", partial(captions, case)) for case in ("one", "multi"))


def dump(out, prefixes):
    from mj_video_amd import ops
    dev = torch.device("cuda:0")
    ops.prof_enable(True)
    for name, run in cases(dev):
        if prefixes and not name.startswith(tuple(prefixes)):
            continue
        d = os.path.join(out, name)
        os.makedirs(d)
        ops.prof_reset()
        with torch.no_grad():
            run(d)
        prof = {k: dict(launches=v["launches"], flops=v["flops"]) for k, v in ops.prof_results().items()}
        json.dump(prof, open(os.path.join(d, "prof.json"), "w"), indent=1, sort_keys=True)
        print(f"{name}: {len(os.listdir(d)) - 1} arrays, {sum(v['launches'] for v in prof.values())} launches", flush=True)
    ops.prof_enable(False)


def compare(a, b) -> int:
    files = {r: sorted(os.path.join(os.path.relpath(p, r), f) for p, _, fs in os.walk(r) for f in fs) for r in (a, b)}
    diffs = [f"{f}: only in {r}" for r, o in ((a, b), (b, a)) for f in files[r] if f not in files[o]]
    both = [f for f in files[a] if f in files[b]]
    for f in both:
        if f.endswith(".json"):
            x, y = (json.load(open(os.path.join(r, f))) for r in (a, b))
            diffs += [f"{f}: {k}: {x.get(k)} != {y.get(k)}" for k in sorted(set(x) | set(y)) if x.get(k) != y.get(k)]
        else:
            x, y = (np.load(os.path.join(r, f)) for r in (a, b))
            if x.shape != y.shape or x.dtype != y.dtype:
                diffs.append(f"{f}: {x.dtype}{x.shape} != {y.dtype}{y.shape}")
            elif x.tobytes() != y.tobytes():
                diffs.append(f"{f}: {int((np.frombuffer(x.tobytes(), np.uint8) != np.frombuffer(y.tobytes(), np.uint8)).sum())} bytes differ")
    print("\n".join(diffs) if diffs else
          f"identical, {len({os.path.dirname(f) for f in both})} cases, {sum(f.endswith('.npy') for f in both)} arrays")
    return 1 if diffs or not both else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--cases", default="")
    ap.add_argument("--compare", nargs=2)
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    dump(args.out, [c for c in args.cases.split(",") if c])
