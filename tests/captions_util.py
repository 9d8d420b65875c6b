"""Inputs of the caption-scoring tests (test infrastructure only): one video under twelve captions, and three videos of
different tile counts under four captions each with an interleaved ``context_index`` - shared by the GPU tests, the host
tests and tests/golden/make_golden_captions.py, so that the stored oracle outputs and the tests speak of the same prompts."""
import os

import numpy as np
import torch

from mj_video_amd import synth
from mj_video_amd.chat_input import num_image_tokens_per_tile

from util import GOLDEN, make_cfg

PIXEL_SEED = 77
ONE_LENGTHS = (1, 4, 9, 16, 24, 32, 40, 48, 64, 96, 128, 160)     # caption i: seed 500 + i, L_i tokens
MULTI_TILES = (8, 6, 3)                                           # video v: video_idx v
MULTI_LENGTHS = (8, 24, 48, 96)                                   # caption j of video v: seed 600 + 4 v + j
ORACLE_FIELDS = ("rewards", "hidden_state", "prompt_embedding", "criteria_gating_output", "aspect_gating_output",
                 "aspect_weights", "score", "weighted_scores", "aspect_scores")
# (dims, image size, tiles of the one-video case)
DIMS = {"tiny": ("tiny", 56, 4), "2b": ("2b", 224, 8)}


def cfg_of(dims: str):
    kind, size, _ = DIMS[dims]
    return make_cfg(kind, size)


def one_case(dims: str):
    """-> (cfg, [pixels of the one video], prompts [1, N_i] x 12, context_index)"""
    kind, size, tiles = DIMS[dims]
    cfg = make_cfg(kind, size)
    per = num_image_tokens_per_tile(cfg)
    px = synth.synth_pixel_values(PIXEL_SEED, 0, tiles, size)
    prompts = [synth.synth_input_ids(tiles * per, 500 + i, n_caption=L) for i, L in enumerate(ONE_LENGTHS)]
    return cfg, [px], prompts, np.zeros(len(prompts), dtype=np.int64)


def multi_case(dims: str):
    """three videos x four captions; row r = 3 j + v (caption-major), so ``context_index`` = 0, 1, 2, 0, 1, 2, ..."""
    kind, size, _ = DIMS[dims]
    cfg = make_cfg(kind, size)
    per = num_image_tokens_per_tile(cfg)
    videos = [synth.synth_pixel_values(PIXEL_SEED, v, t, size) for v, t in enumerate(MULTI_TILES)]
    prompts, index = [], []
    for j, L in enumerate(MULTI_LENGTHS):
        for v, t in enumerate(MULTI_TILES):
            prompts.append(synth.synth_input_ids(t * per, 600 + 4 * v + j, n_caption=L))
            index.append(v)
    return cfg, videos, prompts, np.asarray(index, dtype=np.int64)


CASES = {"one": one_case, "multi": multi_case}


def oracle_outputs(dims: str, case: str, dtype) -> dict:
    """oracle/ref_cpu.reward_forward on the full prompts of the case (right-padded batch, every row with its own video's
    tiles), parameters and pixels in ``dtype``; fields as float32 numpy arrays"""
    from oracle import ref_cpu
    cfg, videos, prompts, index = CASES[case](dims)
    sd = {k: v.to(dtype) for k, v in synth.synth_state_dict(cfg, seed=0).items()}
    ids, mask = synth.pad_batch(prompts)
    px = torch.cat([videos[int(c)] for c in index]).to(dtype)
    out = ref_cpu.reward_forward(sd, cfg, px, ids, mask, synth.IMG_CONTEXT_ID, synth.PAD_ID)
    return {k: out[k].float().numpy() for k in ORACLE_FIELDS}


def golden_path(dims: str, case: str) -> str:
    return os.path.join(GOLDEN, f"captions_{dims}_{case}.npz")


def load_golden_captions(dims: str, case: str):
    """-> (fp32 oracle fields, bf16 oracle fields) of tests/golden/captions_<dims>_<case>.npz"""
    z = np.load(golden_path(dims, case))
    return ({k: z["f32_" + k] for k in ORACLE_FIELDS}, {k: z["bf16_" + k] for k in ORACLE_FIELDS})
