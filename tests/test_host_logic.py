"""CPU: host-side logic of the drop-in boundary (no GPU, no compute calls into the library)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import mj_video_amd
from mj_video_amd import _lib, chat_input, configuration as C, harness, parallel, synth, video
from mj_video_amd.modeling import CustomOutput, InternVLChatRewardModeling, find_token_for_gating
from util import ROOT, make_cfg


# ------------------------------------------------------------------------------------------- C ABI
def test_library_builds_loads_and_exports_every_declared_symbol():
    path = _lib.build_library()
    header = open(os.path.join(ROOT, "include", "mjv.h")).read()
    declared = set(re.findall(r"\b(mjv_[a-z0-9_]+)\s*\(", header))
    assert declared == set(_lib.SYMBOLS), declared ^ set(_lib.SYMBOLS)
    lib = _lib.load_library()
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.mjv_abi_version() == _lib.ABI_VERSION == 7
    assert lib.mjv_arch() == b"gfx950"
    assert os.path.dirname(path).endswith("mj-video_amd")  # in-tree, so the driver sees it loaded
    # ABI 4: no process-wide setter in the product header, and the product library neither exports the measurement switches
    # of the bench build (include/mjv_bench.h) nor contains the kernel variants they select
    assert not [n for n in declared if "_set" in n], [n for n in declared if "_set" in n]
    bench_header = open(os.path.join(ROOT, "include", "mjv_bench.h")).read()
    bench_declared = set(re.findall(r"\b(mjv_bench_[a-z0-9_]+)\s*\(", bench_header))
    assert bench_declared == set(_lib.BENCH_SYMBOLS), bench_declared ^ set(_lib.BENCH_SYMBOLS)
    raw = ctypes.CDLL(path)
    for name in bench_declared:
        assert not hasattr(raw, name), f"{name} exported by the product library"


def test_per_call_choices_are_validated_and_thread_local():
    import threading
    from mj_video_amd import ops
    lib = _lib.load_library()
    d = _lib.GemmDesc()
    d.A = d.W = d.C = 1024
    d.M, d.N, d.K = 4, 8, 64
    d.lda = d.ldw = 64
    d.ldc = 8
    d.tile = 100
    assert lib.mjv_gemm_bf16(ctypes.byref(d), None) == -1 and b"tile" in lib.mjv_last_error()
    a = _lib.AttnDesc()
    a.Q = a.K = a.V = a.O = a.cu_seqlens = 1024
    a.head_dim, a.kernel = 64, 3
    assert lib.mjv_attention_bf16(ctypes.byref(a), None) == -1 and b"kernel" in lib.mjv_last_error()
    # the Python-side defaults are per thread
    ops.gemm_set_tile(128)
    ops.attention_set_variant(5)
    seen = {}

    def other():
        seen["tile"], seen["kernel"], seen["ws"] = ops._tls.tile, ops._tls.attn_kernel, ops._tls.gemm_ws

    t = threading.Thread(target=other)
    t.start()
    t.join()
    try:
        assert seen == {"tile": 0, "kernel": 0, "ws": None} and ops._tls.tile == 128 and ops._tls.attn_kernel == 5
        with pytest.raises(_lib.MjvLibraryError, match="bench build"):
            ops.gemm_set_tile(1003)          # measurement switches do not exist in the product library
        with pytest.raises(_lib.MjvLibraryError, match="bench build"):
            ops.attention_set_variant(2)
    finally:
        ops.gemm_set_tile(0)
        ops.attention_set_variant(0)


def test_library_rejects_bad_arguments_without_a_gpu():
    lib = _lib.load_library()
    d = _lib.GemmDesc()
    assert lib.mjv_gemm_bf16(ctypes.byref(d), None) == -1
    assert b"null pointer" in lib.mjv_last_error()
    d.A = d.W = d.C = 1024
    d.M, d.N, d.K = 4, 8, 100
    d.lda = d.ldw = 104
    d.ldc = 8
    assert lib.mjv_gemm_bf16(ctypes.byref(d), None) == -1
    assert b"multiple of 64" in lib.mjv_last_error()
    a = _lib.AttnDesc()
    a.Q = a.K = a.V = a.O = a.cu_seqlens = 1024
    a.head_dim = 80
    assert lib.mjv_attention_bf16(ctypes.byref(a), None) == -1
    assert b"head_dim" in lib.mjv_last_error()


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(_lib.MjvLibraryError, match="no CPU fallback"):
        _lib.load_library()


def test_product_never_imports_the_oracle():
    """only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may import anything under oracle/: every other
    Python file of the tree (the package, tools/, scripts/) is scanned"""
    allowed_files = {os.path.join(ROOT, "bench.py"), os.path.join(ROOT, "__graft_entry__.py")}
    allowed_dirs = tuple(os.path.join(ROOT, d) + os.sep for d in ("tests", "oracle", "gpurun_out", ".git"))
    seen = 0
    for dirpath, _, files in os.walk(ROOT):
        if (dirpath + os.sep).startswith(allowed_dirs):
            continue
        for f in files:
            path = os.path.join(dirpath, f)
            if f.endswith(".py") and path not in allowed_files:
                seen += 1
                src = open(path).read()
                assert not re.search(r"^\s*(from|import)\s+oracle", src, re.M), path
    assert seen > 20
    # ... and in the two allowed files the import sits inside the function that is allowed to check with it
    for path, fn in ((os.path.join(ROOT, "bench.py"), "cpu_baseline"), (os.path.join(ROOT, "__graft_entry__.py"), "smoke")):
        src = open(path).read()
        for m in re.finditer(r"^(\s*)(from|import)\s+oracle", src, re.M):
            assert m.group(1), (path, "module-level oracle import")
            head = src[:m.start()]
            last_def = re.findall(r"^def (\w+)", head, re.M)[-1]
            assert last_def == fn or fn == "smoke" and last_def.startswith(("smoke", "_smoke")), (path, last_def)


# ------------------------------------------------------------------------------------- prompt logic
class StubTokenizer:
    """duck-typed tokenizer: special tokens are single ids, every other character is one id"""
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
                if text.startswith("assistant", i):      # real tokenizer: 'assistant' -> 525, 11353
                    ids += [525, 11353]
                    i += 9
                elif text[i] == "\n":
                    ids.append(364)
                    i += 1
                else:
                    ids.append(1000 + (ord(text[i]) % 50000))
                    i += 1
        t = torch.tensor([ids])
        return {"input_ids": t, "attention_mask": torch.ones_like(t)}


SYSTEM = ("<|im_start|>system\n你是由上海人工智能实验室联合商汤科技开发的书生多模态大模型，英文名叫InternVL, "
          "是一个有用无害的人工智能助手。<|im_end|>")


def test_prompt_default_only_first_image_placeholder_is_expanded():
    cfg = make_cfg("2b", 448)
    F = 8
    q = chat_input.video_prefix(F) + "a cat"
    s = chat_input.build_query(cfg, q, n_tiles=F)
    ctx = "<IMG_CONTEXT>" * (256 * F)
    expect = (SYSTEM + "<|im_start|>user\nFrame1: <img>" + ctx + "</img>\n" +
              "".join(f"Frame{i}: <image>\n" for i in range(2, F + 1)) + "a cat<|im_end|><|im_start|>assistant\n")
    assert s == expect


def test_prompt_interleaved_and_prefix_rules():
    cfg = make_cfg("2b", 224)
    s = chat_input.build_query(cfg, chat_input.video_prefix(3) + "x", n_tiles=3, num_patches_list=[1, 1, 1])
    assert s.count("<IMG_CONTEXT>") == 3 * 64 and s.count("<img>") == 3 and "<image>" not in s
    s2 = chat_input.build_query(cfg, "describe", n_tiles=2)
    assert "user\n<img>" in s2 and s2.count("<IMG_CONTEXT>") == 128  # '<image>\n' is prepended when missing
    with pytest.raises(AssertionError):
        chat_input.build_query(cfg, "x", n_tiles=3, num_patches_list=[1, 1])


def test_prepare_chat_input_side_effects_and_shapes():
    cfg = make_cfg("2b", 448)
    gen = {"max_new_tokens": 8}
    px = torch.zeros(8, 3, 448, 448)
    ids, mask = chat_input.prepare_chat_input(cfg, StubTokenizer(), px, chat_input.video_prefix(8) + "hi", gen)
    assert gen["eos_token_id"] == 92542
    assert ids.shape == mask.shape and ids.shape[0] == 1
    assert int((ids == 92546).sum()) == 2048
    assert find_token_for_gating(ids[0].tolist()) == ids.shape[1] - 5


def test_find_token_for_gating_matches_reference_semantics():
    pat = [92542, 92543, 525, 11353, 364]
    assert find_token_for_gating([7] + pat + [9] + pat) == 7
    assert find_token_for_gating(pat) == 0
    with pytest.raises(ValueError, match="Token pattern not found in the list."):
        find_token_for_gating([1, 2, 3])
    with pytest.raises(ValueError):
        find_token_for_gating(pat[:-1])


# ------------------------------------------------------------------------------------------ configs
def test_config_roundtrip_and_kwargs_override(tmp_path):
    cfg = make_cfg("2b", 448)
    cfg.save_pretrained(str(tmp_path))
    re_cfg = C.InternVLChatRewardModelingConfig.from_pretrained(str(tmp_path), num_objectives=10, gating_temperature=2.0)
    assert re_cfg.num_objectives == 10 and re_cfg.gating_temperature == 2.0 and re_cfg.num_aspects == 5
    assert re_cfg.aspect2criteria[3] == [16, 17, 18, 19, 20, 21, 22]
    assert re_cfg.llm_config.hidden_size == 2048 and re_cfg.vision_config.patch_size == 14
    assert re_cfg.llm_config.rope_scaling == {"type": "dynamic", "factor": 2.0}
    d = re_cfg.to_dict()
    assert d["model_type"] == "internvl_chat" and d["llm_config"]["num_key_value_heads"] == 8
    with pytest.raises(ValueError, match="rope_scaling"):
        C.InternLM2Config(rope_scaling={"type": "yarn", "factor": 2.0})
    with pytest.raises(ValueError, match="Unsupported architecture"):
        C.InternVLChatConfig(llm_config={"architectures": ["Qwen2ForCausalLM"]})
    assert type(C.InternVLChatConfig(llm_config={"architectures": ["Phi3ForCausalLM"]}).llm_config).__name__ == "Phi3Config"   # configs[4]
    with pytest.raises(FileNotFoundError):
        C.InternVLChatRewardModelingConfig.from_pretrained(str(tmp_path / "missing"))


def test_state_dict_layout_and_param_count():
    cfg = make_cfg("tiny", 56)
    model = InternVLChatRewardModeling.from_config(cfg)
    keys = set(model.state_dict().keys())
    spec = {k: s for k, s, _ in synth.state_dict_spec(cfg)}
    assert keys == set(spec)
    for k, v in model.state_dict().items():
        assert tuple(v.shape) == spec[k], k
    assert "model.mlp1.3.weight" in keys and "model.mlp1.2.weight" not in keys
    assert "model.language_model.output.weight" in keys
    full = make_cfg("2b", 448)
    n = sum(int(np.prod(s)) for k, s, _ in synth.state_dict_spec(full)
            if k.startswith("model."))
    assert n == 2_205_754_368  # matches the published 2.21 B
    with pytest.raises(AssertionError):
        bad = make_cfg("tiny", 56)
        bad.aspect2criteria = {0: [0, 1], 1: [1, 2]}
        InternVLChatRewardModeling.from_config(bad)


def test_checkpoint_directory_ingestion_and_setup_order(tmp_path):
    """``InternVLChatRewardModeling(name, config)`` builds the base model from a local checkpoint
    directory (config.json + sharded *.safetensors, the layout ``InternVLChatModel.from_pretrained`` reads in
    moe_reward.py:142), then the harness order of eval_genai_mjvideo.py:73-116 works: load_state_dict(strict=True) of the
    full reward checkpoint -> pad_token_id -> .to(bf16) -> img_context_token_id -> eval()."""
    from safetensors.torch import save_file
    cfg = make_cfg("tiny", 56)
    cfg.save_pretrained(str(tmp_path))
    sd = synth.synth_state_dict(cfg, seed=3, lm_head=True, dtype=torch.float32)
    base = {k[len("model."):]: v.contiguous() for k, v in sd.items() if k.startswith("model.")}
    keys = sorted(base)
    half = len(keys) // 2
    save_file({k: base[k] for k in keys[:half]}, str(tmp_path / "model-00001-of-00002.safetensors"))
    save_file({k: base[k] for k in keys[half:]}, str(tmp_path / "model-00002-of-00002.safetensors"))
    re_cfg = C.InternVLChatRewardModelingConfig.from_pretrained(str(tmp_path), **{
        k: getattr(cfg, k) for k in ("num_objectives", "num_aspects", "aspect2criteria", "gating_temperature",
                                     "gating_hidden_dim", "gating_n_hidden")})
    model = InternVLChatRewardModeling(str(tmp_path), re_cfg)
    got = model.state_dict()
    for k, v in base.items():
        assert torch.equal(got["model." + k], v), k
    # full reward checkpoint on top, strict, then the reference's set-up order
    missing = model.load_state_dict(sd, strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    model.config.pad_token_id = 2
    model = model.to(torch.bfloat16)
    model.model.img_context_token_id = 92546
    model.eval()
    assert model.model.dtype == torch.bfloat16 and model.regression_layer.weight.dtype == torch.bfloat16
    assert torch.equal(model.state_dict()["regression_layer.weight"], sd["regression_layer.weight"].to(torch.bfloat16))
    # a shard with a key the model does not have is refused (strict), like the reference's load
    save_file({"vision_model.bogus": torch.zeros(1)}, str(tmp_path / "model-00003-of-00002.safetensors"))
    with pytest.raises(RuntimeError, match="bogus"):
        InternVLChatRewardModeling(str(tmp_path), re_cfg)


def test_missing_base_weights_fail_loudly(tmp_path):
    """The reference's ``from_pretrained`` returns real base weights or fails (moe_reward.py:142); a directory without
    ``*.safetensors`` (or a hub name, which cannot be resolved offline) must not yield a torch.empty model silently."""
    from mj_video_amd.modeling import InternVLChatModel
    cfg = make_cfg("tiny", 56)
    cfg.save_pretrained(str(tmp_path))
    with pytest.raises(FileNotFoundError, match="safetensors"):
        InternVLChatRewardModeling(str(tmp_path), cfg)
    with pytest.raises(FileNotFoundError):
        InternVLChatModel.from_pretrained("OpenGVLab/InternVL2-2B", config=cfg)
    skeleton = InternVLChatModel.from_pretrained(str(tmp_path), config=cfg, allow_uninitialized=True)
    assert skeleton.num_image_token == 4


def test_model_refuses_cpu_and_non_bf16():
    cfg = make_cfg("tiny", 56)
    model = InternVLChatRewardModeling.from_config(cfg, dtype=torch.bfloat16)
    model.load_state_dict(synth.synth_state_dict(cfg, seed=1), strict=True)
    model.model.img_context_token_id = synth.IMG_CONTEXT_ID
    with pytest.raises(RuntimeError, match="MI355X only"):
        model.forward(torch.zeros(2, 3, 56, 56, dtype=torch.bfloat16), synth.synth_input_ids(8, 1), None)


def test_token_ids_outside_the_vocabulary_raise():
    """nn.Embedding raises on an id outside [0, vocab) (modeling_internvl_chat.py:161); the gather kernel would read out
    of bounds silently, so the host check stands in for it.  Pad ids in the masked tail are never looked up."""
    cfg = make_cfg("tiny", 56)
    model = InternVLChatRewardModeling.from_config(cfg)
    model.model.img_context_token_id = synth.IMG_CONTEXT_ID
    model.config.pad_token_id = synth.PAD_ID
    vocab = cfg.llm_config.vocab_size
    ids = synth.synth_input_ids(8, 1).numpy().copy()
    model._analyse_ids(ids, None, 2)
    bad = ids.copy()
    bad[0, 5] = vocab
    with pytest.raises(IndexError, match="out of range"):
        model._analyse_ids(bad, None, 2)
    bad[0, 5] = -3
    with pytest.raises(IndexError, match="out of range"):
        model._analyse_ids(bad, None, 2)


def test_analyse_ids_packing():
    cfg = make_cfg("tiny", 56)
    model = InternVLChatRewardModeling.from_config(cfg)
    model.config.pad_token_id = synth.PAD_ID
    model.model.img_context_token_id = synth.IMG_CONTEXT_ID
    a, b = synth.synth_input_ids(16, 1), synth.synth_input_ids(8, 2)
    ids, mask = synth.pad_batch([a, b])
    info = model._analyse_ids(ids.numpy(), mask.numpy().astype(bool), 6)
    assert info["cu"].tolist() == [0, a.shape[1], a.shape[1] + b.shape[1]]
    assert info["sel_rows"].tolist() == [a.shape[1] - 1, a.shape[1] + b.shape[1] - 1, a.shape[1] - 5, a.shape[1] + b.shape[1] - 5]
    assert (info["ids"][info["img_rows"]] == synth.IMG_CONTEXT_ID).all() and info["img_rows"].size == 24
    assert info["positions"][a.shape[1]] == 0
    with pytest.raises(ValueError, match="IMG_CONTEXT"):
        model._analyse_ids(ids.numpy(), mask.numpy().astype(bool), 5)
    # a mask that hides a selected row or an <IMG_CONTEXT> token is refused
    for col in (b.shape[1] - 1, b.shape[1] - 5, int(info["img_rows"][-1]) - a.shape[1]):
        bad = mask.clone()
        bad[1, col] = 0
        with pytest.raises(ValueError, match="masked part"):
            model._analyse_ids(ids.numpy(), bad.numpy().astype(bool), 6)
    # ANY other mask is packed (round 6): LEFT padding - the reference's reward row is then the last column ((first pad) - 1 mod N),
    # positions are the COLUMN indices (modeling_internlm2.py:893-898 numbers positions without looking at the mask)
    pad = a.shape[1] - b.shape[1]
    lids = ids.clone()
    lids[1] = torch.cat([torch.full((pad,), synth.PAD_ID), b[0]])
    lmask = mask.clone()
    lmask[1] = torch.cat([torch.zeros(pad, dtype=mask.dtype), torch.ones(b.shape[1], dtype=mask.dtype)])
    li = model._analyse_ids(lids.numpy(), lmask.numpy().astype(bool), 6)
    assert li["cu"].tolist() == info["cu"].tolist() and (li["ids"] == info["ids"]).all()
    assert li["positions"][a.shape[1]:].tolist() == list(range(pad, a.shape[1]))
    assert li["sel_rows"].tolist() == info["sel_rows"].tolist() and (li["img_rows"] == info["img_rows"]).all()
    # ... and holes: two caption tokens of sample a masked out - they leave the packed rows, the later tokens keep their columns
    hmask = mask.clone()
    hole = [a.shape[1] - 12, a.shape[1] - 9]
    hmask[0, hole] = 0
    hi = model._analyse_ids(ids.numpy(), hmask.numpy().astype(bool), 6)
    keep = [c for c in range(a.shape[1]) if c not in hole]
    assert hi["cu"].tolist() == [0, a.shape[1] - 2, a.shape[1] - 2 + b.shape[1]]
    assert hi["positions"][:a.shape[1] - 2].tolist() == keep and (hi["ids"][:a.shape[1] - 2] == a[0, keep].numpy()).all()
    assert hi["sel_rows"].tolist() == [a.shape[1] - 3, a.shape[1] - 2 + b.shape[1] - 1, a.shape[1] - 7, a.shape[1] - 2 + b.shape[1] - 5]
    assert hi["tail_pos"][:5].tolist() == list(range(a.shape[1] - 5, a.shape[1]))
    model.model.img_context_token_id = None
    with pytest.raises(ValueError, match="img_context_token_id"):
        model._analyse_ids(ids.numpy(), mask.numpy().astype(bool), 6)


def test_analyse_ids_prefix_skip_and_tail():
    """the host side of ABI 6's two trimmings: the common prompt prefix (cut to a multiple of 64, never reaching an <IMG_CONTEXT>
    or a selected row) is offered to the cache lookup and, on a hit, left out of the packed rows while positions keep their
    absolute values; the tail = rows from the first selected one on, with the selected rows' indices inside it"""
    cfg = make_cfg("tiny", 56)
    model = InternVLChatRewardModeling.from_config(cfg)
    model.config.pad_token_id = synth.PAD_ID
    model.model.img_context_token_id = synth.IMG_CONTEXT_ID
    a, b = synth.synth_input_ids(16, 1), synth.synth_input_ids(8, 2)
    ids, mask = synth.pad_batch([a, b])
    ids_np, am = ids.numpy(), mask.numpy().astype(bool)
    La, Lb = a.shape[1], b.shape[1]
    first_ctx = int(np.flatnonzero(ids_np[0] == synth.IMG_CONTEXT_ID)[0])
    assert first_ctx == 71                       # BOS + system turn + "user\n Frame1: <img>" of the synthetic prompt
    seen = []
    info = model._analyse_ids(ids_np, am, 6, lambda p: seen.append(p.copy()) or False)      # offered, refused
    assert len(seen) == 1 and seen[0].tolist() == ids_np[0, :64].tolist() and info["skip"] == 0
    assert info["prefix_ids"].tolist() == ids_np[0, :64].tolist()
    plain = model._analyse_ids(ids_np, am, 6)
    for k in ("ids", "positions", "cu", "img_rows", "sel_rows", "tail_rows", "cu_tail", "sel_in_tail"):
        assert np.array_equal(info[k], plain[k]), k
    assert plain["prefix_ids"] is None and plain["skip"] == 0
    # tail: rows L - 5 .. L - 1 of both samples; reward row = last, gating row = first of the tail
    assert plain["cu_tail"].tolist() == [0, 5, 10] and plain["max_tail"] == 5
    assert plain["tail_rows"].tolist() == list(range(La - 5, La)) + list(range(La + Lb - 5, La + Lb))
    assert plain["tail_pos"].tolist() == list(range(La - 5, La)) + list(range(Lb - 5, Lb))
    assert plain["sel_in_tail"].tolist() == [4, 9, 0, 5]
    hit = model._analyse_ids(ids_np, am, 6, lambda p: True)
    assert hit["skip"] == 64 and hit["total"] == La + Lb - 128 and hit["max_len"] == La - 64
    assert hit["cu"].tolist() == [0, La - 64, La + Lb - 128]
    assert hit["positions"][0] == 64 and hit["positions"][La - 64] == 64 and hit["positions"][La - 65] == La - 1
    assert np.array_equal(hit["ids"], np.concatenate([ids_np[0, 64:La], ids_np[1, 64:Lb]]))
    assert (hit["ids"][hit["img_rows"]] == synth.IMG_CONTEXT_ID).all() and hit["img_rows"].size == 24
    assert hit["sel_rows"].tolist() == [La - 65, La + Lb - 129, La - 69, La + Lb - 133]
    assert hit["tail_rows"].tolist() == list(range(La - 69, La - 64)) + list(range(La + Lb - 133, La + Lb - 128))
    assert hit["tail_pos"].tolist() == plain["tail_pos"].tolist() and hit["sel_in_tail"].tolist() == [4, 9, 0, 5]
    # samples that differ inside the first 64 tokens share no cacheable prefix; a difference at token 70 leaves 64
    other = ids_np.copy()
    other[1, 10] += 1
    assert model._analyse_ids(other, am, 6, lambda p: True)["skip"] == 0
    other = ids_np.copy()
    other[1, 70] += 1
    assert model._analyse_ids(other, am, 6, lambda p: True)["skip"] == 64
    # a 130-token common prefix is cut to 128
    long_a = torch.cat([a[:, :60], a[:, 1:61], a[:, 1:]], dim=1)
    long_b = torch.cat([b[:, :60], b[:, 1:61], b[:, 1:]], dim=1)
    lids, lmask = synth.pad_batch([long_a, long_b])
    assert model._analyse_ids(lids.numpy(), lmask.numpy().astype(bool), 6, lambda p: True)["skip"] == 128


def test_prefix_candidate_on_prompts_built_by_prepare_chat_input():
    """the prompts the eval harness builds (``video_prefix`` + caption through ``prepare_chat_input``, eval_genai_mjvideo.py:132-139) share
    everything up to the first <IMG_CONTEXT>: BOS, the system turn, ``<|im_start|>user\nFrame1: <img>`` - the prefix the cache
    keys on - whatever the captions are; with the stub tokenizer (one id per character) that is 98 tokens, so 64 are cacheable"""
    cfg = make_cfg("tiny", 56)
    model = InternVLChatRewardModeling.from_config(cfg)
    model.config.pad_token_id = 2
    model.model.img_context_token_id = StubTokenizer.special["<IMG_CONTEXT>"]
    tok, rows = StubTokenizer(), []
    for caption in ("a cat sits on a mat", "two dogs run along the beach at dusk, wide shot"):
        ids, _ = chat_input.prepare_chat_input(cfg, tok, torch.zeros(2, 3, 56, 56), chat_input.video_prefix(2) + caption, {})
        rows.append(ids)
    n = max(int(r.shape[1]) for r in rows)
    ids = torch.full((2, n), 2, dtype=torch.long)
    mask = torch.zeros(2, n, dtype=torch.bool)
    for i, r in enumerate(rows):
        ids[i, : r.shape[1]] = r[0]
        mask[i, : r.shape[1]] = True
    first_ctx = [int(np.flatnonzero(ids[i].numpy() == model.model.img_context_token_id)[0]) for i in range(2)]
    assert first_ctx[0] == first_ctx[1] and (ids[0, : first_ctx[0]] == ids[1, : first_ctx[0]]).all()
    per_tile = chat_input.num_image_tokens_per_tile(cfg)
    seen = []
    info = model._analyse_ids(ids.numpy(), mask.numpy(), 4, lambda p: seen.append(len(p)) or True)   # 2 videos x 2 tiles
    assert seen == [(first_ctx[0] // 64) * 64] and info["skip"] == seen[0] > 0
    assert info["img_rows"].size == 2 * 2 * per_tile and (info["ids"][info["img_rows"]] == model.model.img_context_token_id).all()


def test_custom_output_access():
    o = CustomOutput(rewards=torch.ones(1), score=torch.zeros(1))
    assert o["score"] is o.score and o[0] is o.rewards and o.keys() == ["rewards", "score"]


# --------------------------------------------------------------------------------- synthetic inputs
def test_synth_is_deterministic_and_layout_is_right():
    cfg = make_cfg("tiny", 56)
    a = synth.synth_state_dict(cfg, seed=5)
    b = synth.synth_state_dict(cfg, seed=5)
    assert all(torch.equal(a[k], b[k]) for k in a)
    c = synth.synth_state_dict(cfg, seed=6)
    assert not torch.equal(a["regression_layer.weight"], c["regression_layer.weight"])
    # pinned values: any change to the generator silently invalidates every golden vector
    w = synth.synth_state_dict(cfg, seed=11, dtype=torch.float32)["regression_layer.weight"]
    assert abs(float(w[0, 0]) - float(synth._normal(11, "regression_layer.weight", (28, 256), 0.05)[0, 0])) == 0
    ids = synth.synth_input_ids(2048, 3)
    assert ids.shape == (1, 2186) and ids[0, 0] == 1 and ids[0, -5:].tolist() == list(synth.GATING_PATTERN)
    assert int((ids == synth.IMG_CONTEXT_ID).sum()) == 2048 and int((ids == synth.PAD_ID).sum()) == 0
    il = synth.synth_input_ids(32, 3, interleave_frames=4)
    runs = (il[0] == synth.IMG_CONTEXT_ID).int().diff().abs().sum().item()
    assert runs == 8  # four separate runs of context tokens
    px = synth.synth_pixel_values(1, 2, 3, 56)
    assert px.shape == (3, 3, 56, 56) and px.dtype == torch.bfloat16 and torch.equal(px, synth.synth_pixel_values(1, 2, 3, 56))


# -------------------------------------------------------------------------------------- load_video
def test_frame_index_and_tile_grid_pinned_values():
    """values captured from the reference's own functions"""
    assert video.get_index(None, 30.0, 99, 0, 8).tolist() == [0, 12, 24, 37, 49, 61, 74, 86]
    assert video.get_index(None, 30.0, 48, 0, 16).tolist() == [3 * i for i in range(16)]
    assert video.get_index((1.0, 2.0), 10.0, 99, 0, 5).tolist() == [10, 12, 14, 16, 18]
    from PIL import Image

    def ntiles(w, h, max_num):
        return len(video.dynamic_preprocess(Image.new("RGB", (w, h)), image_size=448, use_thumbnail=True, max_num=max_num))

    assert all(ntiles(w, h, 1) == 1 for w, h in [(512, 512), (1280, 720), (720, 1280)])
    assert ntiles(512, 512, 6) == 1 and ntiles(1024, 1024, 6) == 5
    assert [ntiles(w, h, 6) for w, h in [(1280, 720), (1920, 1080), (854, 480), (720, 1280)]] == [3, 3, 3, 3]
    assert ntiles(1344, 896, 6) == 7


def test_load_frames_normalisation_and_order():
    rng = np.random.default_rng(0)
    frames = [rng.integers(0, 256, size=(448, 896, 3), dtype=np.uint8) for _ in range(2)]
    pv, counts = video.load_frames(frames, input_size=448, max_num=2)
    assert counts == [3, 3] and pv.shape == (6, 3, 448, 448) and pv.dtype == torch.float32
    left = torch.from_numpy(frames[0][:, :448].astype(np.float32) / 255.0).permute(2, 0, 1)
    mean = torch.tensor(video.IMAGENET_MEAN).view(3, 1, 1)
    std = torch.tensor(video.IMAGENET_STD).view(3, 1, 1)
    assert torch.allclose(pv[0], (left - mean) / std, atol=1e-6)  # 2x1 grid at native size: first tile = left half
    pv1, c1 = video.load_frames(frames, input_size=448, max_num=1)
    assert c1 == [1, 1] and pv1.shape == (2, 3, 448, 448)
    with pytest.raises(RuntimeError, match="no network"):
        video.load_video("http://example.com/x.mp4")


def test_pil_resize_restatement_is_bit_exact():
    """the integer restatement that feeds the GPU preprocessing kernel reproduces Pillow's own bicubic resize bit for bit
    (down- and up-scaling, both axes, identity)"""
    from PIL import Image
    rng = np.random.default_rng(3)
    for (H, W, ow, oh) in [(360, 640, 448, 448), (96, 128, 448, 448), (270, 480, 896, 448), (448, 448, 448, 448), (500, 333, 448, 896)]:
        img = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
        ref = np.asarray(Image.fromarray(img).resize((ow, oh)))
        assert np.array_equal(video.pil_resize_u8(img, ow, oh), ref), (H, W, ow, oh)
    b, k = video.pil_resample_coeffs(1280, 448)
    assert k.shape == (448, 13) and b[0].tolist() == [0, 7] and int(k[100].sum()) in range((1 << 22) - 8, (1 << 22) + 8)


# ----------------------------------------------------------------------------------------- harness
def test_preference_protocol():
    votes = [("rightvote", 0.1, 0.5), ("rightvote", 0.5, 0.1), ("leftvote", 0.3, -0.2), ("bothbad_vote", -1.0, -0.1),
             ("bothbad_vote", -1.0, 0.1), ("tievote", 0.2, 0.3), ("tievote", 0.2, 0.0), ("leftvote", 0.1, 0.1)]
    c = harness.evaluate_votes(votes)
    assert (c.prefer_truth, c.prefer_total, c.truth, c.total) == (2, 4, 4, 8)
    assert c.prefer_acc == 0.5 and c.acc == 0.5


def test_label_schema_mappings():
    assert harness.criteria_targets({"a": 1, "b": 2, "c": 0, "d": 3}) == ([1, -1, 0, 0], [1, 1, 0, 0], ["a", "b", "c", "d"])
    assert harness.criteria_targets({"a": 2}, mse=False)[0] == [0]
    assert harness.overall_target(1) == ([1], [1]) and harness.overall_target(2) == ([-1], [1]) and harness.overall_target(0) == ([0], [0])
    assert harness.preference_targets({"x": "Video 1 better", "y": "Video 2 better", "z": "tie"}) == ([0, 1, 1], [1, 1, 0])
    assert harness.preference_targets("Video 2 better") == ([1], [1])
    # the label file shipped with the reference parses with these rules (its first record, stored in tests/golden/label_record.json)
    import json
    rec = json.load(open(os.path.join(ROOT, "tests", "golden", "label_record.json")))
    for key in ("video_0_label", "video_1_label"):
        s, r, names = harness.criteria_targets(rec[key])
        assert len(s) == len(r) == len(names) == 28 and set(s) <= {-1, 0, 1}


def test_shard_bounds_cover_everything():
    for n in (0, 1, 7, 64):
        for w in (1, 2, 8):
            spans = [parallel.shard_bounds(n, w, r) for r in range(w)]
            assert spans[0][0] == 0 and spans[-1][1] == n
            assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
            assert max(b - a for a, b in spans) - min(b - a for a, b in spans) <= 1


def test_dropin_import_paths():
    import importlib
    import sys
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        m = importlib.import_module("model")
        assert m.InternVLChatRewardModelingConfig is C.InternVLChatRewardModelingConfig
        assert m.prepare_chat_input is chat_input.prepare_chat_input
        dp = importlib.import_module("data_processor")
        assert dp.load_video is video.load_video
    finally:
        sys.path.remove(os.path.join(ROOT, "scripts"))


def test_load_video_end_to_end_with_a_stub_decoder(monkeypatch):
    """data.py:158-179 end to end: ``load_video`` = decode (decord.VideoReader) -> get_index -> per frame dynamic_preprocess +
    transform -> stacked tiles.  decord is not installed in this image, so a stub module with the three things the path uses
    (``VideoReader(path, ctx, num_threads)``, ``len``, ``get_avg_fps``, ``vr[i].asnumpy()``) stands in: the run must sample
    exactly the frames ``get_index`` names (the index function itself is pinned to the reference's, tests/golden/host.json),
    honour ``bound``, and return the tiles ``load_frames`` gives for those frames."""
    import sys
    import types

    n_frames, fps, H, W = 50, 10.0, 72, 96
    rng = np.random.default_rng(3)
    clip = rng.integers(0, 256, size=(n_frames, H, W, 3), dtype=np.uint8)
    opened = []

    class _Frame:
        def __init__(self, a):
            self.a = a

        def asnumpy(self):
            return self.a

    class VideoReader:
        def __init__(self, path, ctx=None, num_threads=0):
            opened.append((path, ctx, num_threads))
            self.read = []

        def __len__(self):
            return n_frames

        def get_avg_fps(self):
            return fps

        def __getitem__(self, i):
            self.read.append(int(i))
            return _Frame(clip[int(i)])

    stub = types.ModuleType("decord")
    stub.VideoReader, stub.cpu = VideoReader, (lambda i=0: ("cpu", i))
    monkeypatch.setitem(sys.modules, "decord", stub)

    for bound, segs, max_num in ((None, 8, 1), ((1.0, 3.5), 4, 1), (None, 3, 4)):
        idx = video.get_index(bound, fps, n_frames - 1, first_idx=0, num_segments=segs)
        px, patches = video.load_video("/videos/clip.mp4", bound=bound, input_size=56, max_num=max_num, num_segments=segs)
        want_px, want_patches = video.load_frames([clip[int(i)] for i in idx], input_size=56, max_num=max_num)
        assert patches == want_patches and len(patches) == segs
        assert torch.equal(px, want_px) and px.shape[0] == sum(patches) and px.shape[1:] == (3, 56, 56)
        frames = video.decode_frames("/videos/clip.mp4", bound=bound, num_segments=segs)
        assert frames.shape == (segs, H, W, 3) and np.array_equal(frames, clip[np.asarray(idx, dtype=int)])
    assert all(p == "/videos/clip.mp4" and n == 1 for p, _, n in opened)
    with pytest.raises(RuntimeError, match="no network"):
        video.load_video("https://example.com/clip.mp4")


def test_persistent_gemm_counted_wait_matches_the_emitted_stores():
    """gemm256p_kernel waits for the prefetched K-tile with s_waitcnt vmcnt(N), N = the previous tile's pass-B stores + the 4
    LDS-DMA instructions issued behind the prefetch: a wait for the DMA that does not also drain the stores.  N is spelled out
    in the source (20 / 12), so it has to be checked against what the compiler actually emitted: per persistent
    instantiation, the number of 16-byte store instructions per tile - each store site is a plain arm and an inline-asm nt arm,
    exactly one of which executes - must be N - 4."""
    import re
    import subprocess
    import tempfile
    from mj_video_amd import _lib
    src = os.path.join(_lib.CSRC_DIR, "gemm.hip")
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "gemm.s")
        r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", f"-I{os.path.join(ROOT, 'include')}",
                            f"-I{_lib.CSRC_DIR}", "-S", "--cuda-device-only", src, "-o", out], stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout[-2000:]
        text = open(out).read()
    kernels = re.findall(r"^(_ZN\S*gemm256p_kernel\S*):.*?\.end_amdhsa_kernel", text, re.S | re.M)
    bodies = {m.group(1): m.group(0) for m in re.finditer(r"^(_ZN\S*gemm256p_kernel\S*):.*?\.end_amdhsa_kernel", text, re.S | re.M)}
    assert len(bodies) >= 3 and len(kernels) == len(bodies)
    for name, body in bodies.items():
        plain = len(re.findall(r"global_store_dwordx4 [^\n]*off\s*$", body, re.M))
        nt = len(re.findall(r"global_store_dwordx4 [^\n]*off nt\s*$", body, re.M))
        waits = sorted({int(w) for w in re.findall(r"s_waitcnt vmcnt\((\d+)\)", body)})
        assert plain == nt and plain in (8, 16), (name, plain, nt)
        assert waits == [0, 4, plain + 4], (name, plain, waits)


def test_scoring_entry_points_refuse_the_bench_library(monkeypatch):
    from mj_video_amd import _lib
    _lib.load_library()
    assert not _lib.is_bench_build()
    _lib.assert_product_library()
    monkeypatch.setattr(_lib, "is_bench_build", lambda: True)
    with pytest.raises(_lib.MjvLibraryError, match="diagnostics build"):
        _lib.assert_product_library()
    # a library from any other path is refused too (the stamps build exports no bench symbol: ADVICE r4)
    monkeypatch.setattr(_lib, "is_bench_build", lambda: False)
    # what counts is the file load_library() OPENED, not what MJV_LIBRARY says at check time: a variable set or
    # changed after the load neither hides a diagnostics build nor condemns the product library
    stamps = os.path.join(os.path.dirname(_lib.LIB_PATH), "libmjv_hip_stamps.so")
    monkeypatch.setenv("MJV_LIBRARY", stamps)
    _lib.assert_product_library()
    monkeypatch.delenv("MJV_LIBRARY")
    monkeypatch.setattr(_lib, "_lib_path", os.path.realpath(stamps))
    with pytest.raises(_lib.MjvLibraryError, match="diagnostics build"):
        _lib.assert_product_library()
    monkeypatch.setattr(_lib, "_lib_path", os.path.realpath(_lib.LIB_PATH))
    _lib.assert_product_library()
    # ... and the harness entry points call it before they touch the model
    monkeypatch.setattr(_lib, "is_bench_build", lambda: True)
    with pytest.raises(_lib.MjvLibraryError, match="diagnostics build"):
        harness.score_pair_batch(None, None, None, [], {})
    with pytest.raises(_lib.MjvLibraryError, match="diagnostics build"):
        harness.score_collated_batch(None, {})


def test_committed_gelu_table_equals_torch_for_every_bf16_input():
    """mj-video_amd/csrc/gelu_table.h (generated, committed) restated on the CPU: |x| bits < LO -> x / 2, >= HI -> x / -0, else the
    table - equal to torch's bf16 GELU (erf form: F.gelu on the bf16 Linear output, modeling_intern_vit.py:259-261) for every
    finite bf16 input whose half is normal.  The GPU suite checks the KERNELS on every input; this pins the table itself, and the
    window the GEMM epilogue's fast path relies on (2^-23 <= |x| < 128: real activations stay inside it)."""
    import re
    src = open(os.path.join(ROOT, "mj-video_amd", "csrc", "gelu_table.h")).read()
    val = lambda name: int(re.search(rf"#define {name} (\S+)", src).group(1), 0)   # noqa: E731
    LO, HI, R, NEG, LEN = val("MJV_GELU_LO"), val("MJV_GELU_HI"), val("MJV_GELU_R"), val("MJV_GELU_NEG_OFF"), val("MJV_GELU_TABLE_LEN")
    body = src[src.index("MJV_GELU_TABLE_INIT {"):]
    tab = np.array([int(t, 16) for t in re.findall(r"0x[0-9a-f]{4}", body)], dtype=np.int64)
    assert len(tab) == LEN and R == HI - LO and NEG >= R and NEG % 8 == 0 and LEN >= NEG + R and LEN % 8 == 0
    assert LO <= 0x3400 and HI >= 0x4300, "the fast path's window: 2^-23 <= |x| < 128"
    bits = np.arange(65536, dtype=np.int64)
    x = torch.from_numpy(bits.astype(np.uint16).view(np.int16)).view(torch.bfloat16)
    want = torch.nn.functional.gelu(x).view(torch.int16).numpy().astype(np.int64) & 0xFFFF
    half = (x.float() * 0.5).to(torch.bfloat16).view(torch.int16).numpy().astype(np.int64) & 0xFFFF
    mag, sign = bits & 0x7FFF, bits >> 15
    # beyond the table (mjv_common.h gelu_beyond_table): x, +inf once 2 x overflows fp32, -0 for finite x < 0, NaN for +-inf, NaN kept
    beyond = np.where(mag >= 0x7F80, np.where(mag == 0x7F80, np.where(sign == 1, 0x7FC0, 0xFFC0), bits | 0x0040),
                      np.where(sign == 1, 0x8000, np.where(mag >= 0x7F00, 0x7F80, bits)))
    got = np.where(mag < LO, half, np.where(mag >= HI, beyond, tab[np.clip(mag - LO, 0, R - 1) + sign * NEG]))
    check = mag >= 0x0100      # every input whose half is a normal number (as tools/gen_gelu_table.py) - infinities and NaNs included
    assert np.array_equal(got[check], want[check]), int((got[check] != want[check]).sum())


# ------------------------------------------------------------------------------------------- bench.py --dump-outputs
def test_bench_dump_outputs_float32_and_capped(tmp_path):
    """bench.dump_outputs: every array as a float32 .npy, values unchanged; past the byte cap the same seeded rows of every
    array with as many rows, the same in every run, and the files stay under the cap"""
    import bench
    g = torch.Generator().manual_seed(0)
    small = {"packed34": torch.randn(4, 2, 34, generator=g), "hidden_state": torch.randn(8, 2048, generator=g).to(torch.bfloat16)}
    assert bench.dump_outputs(str(tmp_path / "small"), small) == {"packed34": [4, 2, 34], "hidden_state": [8, 2048]}
    for k, v in small.items():
        a = np.load(tmp_path / "small" / f"{k}.npy")
        assert a.dtype == np.float32 and np.array_equal(a, v.float().numpy())
    big = {"a": torch.randn(4096, 1024, generator=g), "b": torch.randn(4096, 256, generator=g).to(torch.bfloat16)}   # 20 MiB in fp32
    cap = 4 << 20
    for run in ("r1", "r2"):
        shapes = bench.dump_outputs(str(tmp_path / run), big, max_bytes=cap)
        assert shapes["a"][1:] == [1024] and shapes["b"][1:] == [256] and 1 <= shapes["a"][0] == shapes["b"][0] < 4096
        assert sum(os.path.getsize(tmp_path / run / f) for f in os.listdir(tmp_path / run)) <= cap
    a, b = (np.load(tmp_path / "r1" / f"{k}.npy") for k in "ab")
    rows = {float(x): i for i, x in enumerate(big["a"][:, 0].numpy())}
    idx = [rows[float(x)] for x in a[:, 0]]
    assert idx == sorted(set(idx)) and np.array_equal(a, big["a"].numpy()[idx]) and np.array_equal(b, big["b"].float().numpy()[idx])
    assert all(np.array_equal(np.load(tmp_path / "r1" / f"{k}.npy"), np.load(tmp_path / "r2" / f"{k}.npy")) for k in "ab")
