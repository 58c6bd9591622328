"""The text encoder without a GPU: the tokenizer against hand-worked ids and against transformers, the module tree against
transformers and against an fp64 restatement written here, the published parameter counts, the load contract, the C ABI's argument
checks, the route ledger, and a prompt as the unconditional input of image sampling on the host."""
import ctypes
import inspect
import json
import math

import pytest
import torch

import _attn_cases as A
import _text_cases as T

BOS, EOS = "<|startoftext|>", "<|endoftext|>"

# ---------------------------------------------------------------------------------------------------------------------
# tokenizer
# ---------------------------------------------------------------------------------------------------------------------
VOCAB = ["!", "!</w>", "a", "a</w>", "b", "b</w>", "'", "s</w>", "l", "l</w>", "1</w>", "2</w>",
         "ab", "ab</w>", "'s</w>", "ll</w>", "'ll</w>", "!!</w>", BOS, EOS]                  # id = position; BOS 18, EOS 19
MERGES = [("a", "b</w>"), ("a", "b"), ("'", "s</w>"), ("l", "l</w>"), ("'", "ll</w>"), ("!", "!</w>")]
# worked by hand: split pattern -> symbols with </w> on the last -> merges by rank
HAND = [
    ("", []),
    ("AB  aB", [13, 13]),                    # lower-cased, spaces collapsed; (a, b</w>) is rank 0 -> "ab</w>"
    ("  a   b ", [3, 5]),
    ("aba", [12, 3]),                        # (a, b, a</w>): only (a, b) is a merge -> "ab", "a</w>"
    ("ab's", [13, 14]),                      # "ab" | "'s": (', s</w>) -> "'s</w>"
    ("A'LL", [3, 16]),                       # "a" | "'ll": (l, l</w>) rank 3 first, then (', ll</w>) rank 4
    ("12", [10, 11]),                        # one digit per token
    ("!!!", [0, 17]),                        # one punctuation run: (!, !, !</w>) -> (!, !!</w>); (!, !) is no merge
    ("a! b", [3, 1, 5]),
    ("ab12!!", [13, 10, 11, 17]),
]
ASCII_STRINGS = [s for s, _ in HAND] + ["a " * 100, "ab " * 40 + "b's 12 !!"]


def _write_tokenizer(path, pad=None):
    path.mkdir(parents=True, exist_ok=True)
    (path / "vocab.json").write_text(json.dumps({t: i for i, t in enumerate(VOCAB)}))
    (path / "merges.txt").write_text("#version: 0.2\n" + "".join(f"{a} {b}\n" for a, b in MERGES))
    if pad is not None:
        (path / "special_tokens_map.json").write_text(json.dumps({"pad_token": pad}))
    return path


def test_tokenizer_hand_worked(tmp_path):
    from stablekeypoints_amd.ldm.tokenizer import CLIPTokenizer
    tok = CLIPTokenizer.from_dir(str(_write_tokenizer(tmp_path / "sd1")))
    assert (tok.bos_token_id, tok.eos_token_id, tok.pad_token_id, len(tok)) == (18, 19, 19, 20)
    for text, ids in HAND:
        assert tok.encode(text) == [18] + ids + [19], text
    out = tok([t for t, _ in HAND], padding="max_length", max_length=77, return_tensors="pt").input_ids
    assert out.dtype == torch.long and out.shape == (len(HAND), 77)
    for row, (_, ids) in zip(out.tolist(), HAND):
        assert row == [18] + ids + [19] * (76 - len(ids))                       # EOS, then EOS as the pad (SD-1.x)
    long = tok(["a " * 100], padding="max_length", max_length=77, return_tensors="pt").input_ids[0].tolist()
    assert long == [18] + [3] * 75 + [19]                                        # cut to 77, EOS stays last
    assert tok("a " * 100, max_length=5).input_ids == [18, 3, 3, 3, 19]
    # the other pad convention: "!" = id 0 (SD-2.x, SDXL's second tokenizer), named by the file beside the vocabulary
    tok2 = CLIPTokenizer.from_dir(str(_write_tokenizer(tmp_path / "sd2", pad="!")))
    assert tok2.pad_token_id == 0
    assert tok2(["ab"], padding="max_length", max_length=6, return_tensors="pt").input_ids.tolist() == [[18, 13, 19, 0, 0, 0]]
    assert tok2.encode("a!! b!") == [18, 3, 0, 0, 5, 0, 19]       # there "!" is a special token: cut out of the text, never merged
    (tmp_path / "sd3").mkdir()
    (tmp_path / "sd3" / "tokenizer_config.json").write_text(json.dumps({"pad_token": {"content": "!"}}))
    _write_tokenizer(tmp_path / "sd3")
    assert CLIPTokenizer.from_dir(str(tmp_path / "sd3")).pad_token_id == 0
    with pytest.raises(FileNotFoundError, match="merges.txt"):
        (tmp_path / "sd3" / "merges.txt").unlink()
        CLIPTokenizer.from_dir(str(tmp_path / "sd3"))


def test_tokenizer_byte_level_vocabulary(tmp_path):
    from stablekeypoints_amd.ldm.tokenizer import CLIPTokenizer
    tok = CLIPTokenizer.byte_level()
    assert len(tok) == 514 and (tok.bos_token_id, tok.eos_token_id, tok.pad_token_id) == (512, 513, 513)
    assert tok.encode("Hi a") == [512, ord("h"), 256 + ord("i"), 256 + ord("a"), 513]
    assert tok.encode("é") == [512, 0xC3, 256 + 0xA9, 513]                       # any byte string is encodable
    tok.save(str(tmp_path / "t"))
    again = CLIPTokenizer.from_dir(str(tmp_path / "t"))
    assert again.encoder == tok.encoder and again.merges == [] and again.pad_token_id == 513


def _hf_tokenizer(path, pad):
    from transformers import CLIPTokenizer as HF
    if "vocab_file" in inspect.signature(HF.__init__).parameters:
        return HF(vocab_file=str(path / "vocab.json"), merges_file=str(path / "merges.txt"), pad_token=pad)
    return HF(vocab=str(path / "vocab.json"), merges=str(path / "merges.txt"), pad_token=pad)


def test_tokenizer_against_transformers(tmp_path):
    pytest.importorskip("transformers")
    from stablekeypoints_amd.ldm.tokenizer import CLIPTokenizer
    for name, pad in (("sd1", EOS), ("sd2", "!")):
        path = _write_tokenizer(tmp_path / name, pad=pad)
        own, hf = CLIPTokenizer.from_dir(str(path)), _hf_tokenizer(path, pad)
        want = hf(ASCII_STRINGS, padding="max_length", max_length=77, truncation=True, return_tensors="pt").input_ids
        got = own(ASCII_STRINGS, padding="max_length", max_length=77, return_tensors="pt").input_ids
        assert torch.equal(got, want), [s for s, a, b in zip(ASCII_STRINGS, got, want) if not torch.equal(a, b)]
    # and the built-in byte vocabulary, where every ASCII string is in the vocabulary
    own = CLIPTokenizer.byte_level()
    own.save(str(tmp_path / "bytes"))
    hf = _hf_tokenizer(tmp_path / "bytes", EOS)
    texts = ASCII_STRINGS + ["Hello  World", "it's we'll I'VE", "abc123", "wow!!! ...ok?", "under_score __ a_b", "a photo of a cat"]
    want = hf(texts, padding="max_length", max_length=77, truncation=True, return_tensors="pt").input_ids
    assert torch.equal(own(texts, padding="max_length", max_length=77, return_tensors="pt").input_ids, want)


# ---------------------------------------------------------------------------------------------------------------------
# module tree
# ---------------------------------------------------------------------------------------------------------------------
def restate64(sd, ids, heads, act, eos, projected):
    """The tower in fp64 from a state dict: embedding, pre-LN blocks, causal softmax -> (last, penultimate, pooled)."""
    w = {k: v.double() for k, v in sd.items()}
    F = torch.nn.functional
    n, L = ids.shape
    x = w["text_model.embeddings.token_embedding.weight"][ids] + w["text_model.embeddings.position_embedding.weight"][:L]
    width = x.shape[-1]
    d = width // heads
    layers = 1 + max(int(k.split(".")[3]) for k in w if k.startswith("text_model.encoder.layers."))
    mask = torch.full((L, L), float("-inf"), dtype=torch.float64).triu(1)
    hidden = [x]
    for i in range(layers):
        p = f"text_model.encoder.layers.{i}."
        h = F.layer_norm(x, (width,), w[p + "layer_norm1.weight"], w[p + "layer_norm1.bias"], 1e-5)
        q, k, v = ((h @ w[p + f"self_attn.{t}_proj.weight"].T + w[p + f"self_attn.{t}_proj.bias"]).view(n, L, heads, d).transpose(1, 2)
                   for t in "qkv")
        a = torch.softmax(q @ k.transpose(-1, -2) * d ** -0.5 + mask, dim=-1) @ v
        x = x + a.transpose(1, 2).reshape(n, L, width) @ w[p + "self_attn.out_proj.weight"].T + w[p + "self_attn.out_proj.bias"]
        h = F.layer_norm(x, (width,), w[p + "layer_norm2.weight"], w[p + "layer_norm2.bias"], 1e-5)
        h = h @ w[p + "mlp.fc1.weight"].T + w[p + "mlp.fc1.bias"]
        h = h * torch.sigmoid(1.702 * h) if act == "quick_gelu" else 0.5 * h * (1 + torch.erf(h / math.sqrt(2)))
        x = x + h @ w[p + "mlp.fc2.weight"].T + w[p + "mlp.fc2.bias"]
        hidden.append(x)
    last = F.layer_norm(x, (width,), w["text_model.final_layer_norm.weight"], w["text_model.final_layer_norm.bias"], 1e-5)
    first_eos = (ids == eos).int().argmax(-1)
    pooled = last[torch.arange(n), first_eos]
    if projected:
        pooled = pooled @ w["text_projection.weight"].T
    return last, hidden[-2], pooled


@pytest.mark.parametrize("act", ["quick_gelu", "gelu"])
@pytest.mark.parametrize("projected", [False, True])
def test_tree_against_fp64_restatement(act, projected):
    m = T.tower(128, 2, act, projection_dim=64 if projected else None)
    ids = T.prompt_ids()
    last, pooled = m(ids)
    pen, pooled2 = m(ids, penultimate=True)
    assert isinstance(m(ids), tuple) and last.shape == (3, 77, 128) and pooled.shape == (3, 64 if projected else 128)
    assert torch.equal(pooled, pooled2) and not last.requires_grad
    want = restate64(m.state_dict(), ids, 2, act, 513, projected)
    m64 = T.tower(128, 2, act, projection_dim=64 if projected else None).double()
    for got, got64, ref, what in ((last, m64(ids)[0], want[0], "last"), (pen, m64(ids, penultimate=True)[0], want[1], "penultimate"),
                                  (pooled, m64(ids)[1], want[2], "pooled")):
        # the tree in fp64 IS the restatement up to fp64 rounding; in fp32 within fp32 rounding of a 2-layer tower (outputs are O(1):
        # 1e-5 is ~100 ulp, far below any structural difference such as a missing mask, norm or activation)
        assert (got64 - ref).abs().max().item() < 1e-12, what
        assert (got.double() - ref).abs().max().item() < 1e-5, what


# 2 x the largest |fp32 - fp64| of transformers' own run of these four models (seed 3, T.prompt_ids()) over the three outputs.
# Measured here: last hidden 2.315e-6 (quick_gelu) / 1.807e-6 (gelu), penultimate 1.089e-6 / 1.029e-6, pooled 1.328e-6 / 1.453e-6,
# projected 1.084e-6 / 1.317e-6; outputs up to 3.7 in magnitude.  Largest: 2.315e-6.
HF_TOL = 2 * 2.315e-6


@pytest.mark.parametrize("act", ["quick_gelu", "gelu"])
@pytest.mark.parametrize("projected", [False, True])
def test_tree_against_transformers(act, projected):
    tf = pytest.importorskip("transformers")
    from stablekeypoints_amd.ldm.clip import CLIPTextModel, canonical_keys, kwargs_from_config
    from stablekeypoints_amd.ldm.pipeline import load_checked
    cfg = tf.CLIPTextConfig(vocab_size=514, hidden_size=128, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2,
                            max_position_embeddings=77, hidden_act=act, projection_dim=64, bos_token_id=512, eos_token_id=513,
                            pad_token_id=513)
    torch.manual_seed(3)
    hf = (tf.CLIPTextModelWithProjection if projected else tf.CLIPTextModel)(cfg).eval()
    own = CLIPTextModel(**kwargs_from_config(cfg.to_dict(), projected))
    state = canonical_keys(hf.state_dict())           # (transformers >= 5 drops the `text_model.` prefix in memory, not in checkpoints)
    load_checked(own, state, "transformers state dict", ("text_model.embeddings.position_ids",))             # no missing, no unexpected
    assert set(own.state_dict()) == set(state) - {"text_model.embeddings.position_ids"}
    ids = T.prompt_ids()
    with torch.no_grad():
        o = hf(input_ids=ids, output_hidden_states=True)
    want = (o.last_hidden_state, o.hidden_states[-2], o.text_embeds if projected else o.pooler_output)
    last, pooled = own(ids)
    pen, _ = own(ids, penultimate=True)
    for got, ref, what in ((last, want[0], "last"), (pen, want[1], "penultimate"), (pooled, want[2], "pooled")):
        diff = (got - ref).abs().max().item()
        print(f"tree vs transformers {act} projected={projected} {what}: {diff:.3e}")
        assert got.shape == ref.shape and diff <= HF_TOL, (what, diff)


def test_published_parameter_counts():
    from stablekeypoints_amd.ldm.clip import CLIPTextModel, CONFIGS, n_params
    want = {"sd15": 123_060_480, "sd21": 340_387_840, "sdxl_2": 694_659_840}
    for name, n in want.items():
        with torch.device("meta"):
            m = CLIPTextModel(**CONFIGS[name])
        assert n_params(m) == n, (name, n_params(m))
        assert hasattr(m, "text_projection") == (name == "sdxl_2")


# ---------------------------------------------------------------------------------------------------------------------
# load contract
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny_pair():
    from stablekeypoints_amd.optimize_token import load_ldm
    plain, pc, _ = load_ldm("cpu", "tiny", feature_upsample_res=32, decoder=True)
    full, fc, _ = load_ldm("cpu", "tiny", feature_upsample_res=32, decoder=True, text_encoder=True)
    return plain, next(iter(pc.values())), full, next(iter(fc.values()))


def test_default_load_has_no_text_encoder(tiny_pair):
    from stablekeypoints_amd.optimize_token import load_ldm
    plain, _, full, _ = tiny_pair
    bare, _, _ = load_ldm("cpu", "tiny", feature_upsample_res=32)
    for m in (plain, bare):
        assert not hasattr(m, "tokenizer") and not hasattr(m, "text_encoder_2")
        with pytest.raises(RuntimeError, match="not on the token-optimisation path"):
            m.text_encoder(torch.zeros(1, 77, dtype=torch.long))
    for a, b in ((plain.unet, full.unet), (plain.vae, full.vae)):
        sa, sb = a.state_dict(), b.state_dict()
        assert list(sa) == list(sb)
        for k in sa:
            assert torch.equal(sa[k], sb[k]), k
    assert all(not p.requires_grad for p in full.text_encoder.parameters())
    assert len(full.tokenizer) == 514


@pytest.mark.parametrize("arch", ["tiny", "tiny-sd21", "tiny-sdxl"])
def test_encode_prompt_shapes_and_reference_call(arch):
    from stablekeypoints_amd import ptp_utils
    from stablekeypoints_amd.optimize_token import load_ldm
    ldm, _, _ = load_ldm("cpu", arch, feature_upsample_res=32, text_encoder=True)
    D = ldm.unet.config["cross_attention_dim"]
    got = ptp_utils.encode_prompt(ldm, ["a photo"])
    # the reference's call, ptp_utils.py:436-439
    ids = ldm.tokenizer(["a photo"], padding="max_length", max_length=77, return_tensors="pt").input_ids
    assert ids.shape == (1, 77) and ids.dtype == torch.long
    if arch == "tiny-sdxl":
        ctx, pooled = got
        ids2 = ldm.tokenizer_2(["a photo"], padding="max_length", max_length=77, return_tensors="pt").input_ids
        h2, p2 = ldm.text_encoder_2(ids2, penultimate=True)
        assert torch.equal(ctx, torch.cat([ldm.text_encoder(ids, penultimate=True)[0], h2], dim=-1))
        assert pooled.shape == (1, ldm.text_encoder_2.config["projection_dim"]) and torch.equal(pooled, p2)
        assert all(not p.requires_grad for p in ldm.text_encoder_2.parameters())
    else:
        ctx = got
        assert torch.equal(ctx, ldm.text_encoder(ids)[0])
    assert ctx.shape == (1, 77, D) and ctx.dtype == torch.float32
    one = ptp_utils.encode_prompt(ldm, "a photo")                                         # a plain string is one prompt
    assert torch.equal(one[0] if isinstance(one, tuple) else one, ctx)
    two = ptp_utils.encode_prompt(ldm, ["a photo", ""])
    two = two[0] if isinstance(two, tuple) else two
    # (a batch of two runs other GEMM blockings than a batch of one: the same row to fp32 rounding, not to the bit)
    assert two.shape == (2, 77, D) and (two[:1] - ctx).abs().max().item() < 1e-5


def test_checkpoint_directory_round_trip(tmp_path, tiny_pair):
    import stablekeypoints_amd.ldm.pipeline as P
    from stablekeypoints_amd import ptp_utils
    from stablekeypoints_amd.optimize_token import load_ldm
    _, _, full, _ = tiny_pair
    d = tmp_path / "tiny-ckpt"
    (d / "text_encoder").mkdir(parents=True)
    torch.save(full.unet.state_dict(), str(d / "unet.pt"))
    torch.save(full.vae.state_dict(), str(d / "vae.pt"))
    orig = P.guess_arch
    P.guess_arch = lambda name: "tiny"
    try:
        with pytest.raises(FileNotFoundError, match="text_encoder"):
            load_ldm("cpu", str(d), feature_upsample_res=32, text_encoder=True)           # no weights yet
        load_ldm("cpu", str(d), feature_upsample_res=32)                                   # not asked for: not needed
        state = dict(full.text_encoder.state_dict())
        state["text_model.embeddings.position_ids"] = torch.arange(77)[None]               # the old buffer is tolerated
        torch.save(state, str(d / "text_encoder" / "pytorch_model.bin"))
        (d / "text_encoder" / "config.json").write_text(json.dumps(full.text_encoder.config))
        with pytest.raises(FileNotFoundError, match="tokenizer"):
            load_ldm("cpu", str(d), feature_upsample_res=32, text_encoder=True)
        full.tokenizer.save(str(d / "tokenizer"))
        back, _, _ = load_ldm("cpu", str(d), feature_upsample_res=32, decoder=False, text_encoder=True)
        assert not back.synthetic_weights and all(not p.requires_grad for p in back.text_encoder.parameters())
        for k, v in full.text_encoder.state_dict().items():
            assert torch.equal(back.text_encoder.state_dict()[k], v), k
        assert torch.equal(ptp_utils.encode_prompt(back, ["a cat's 2 hats!"]), ptp_utils.encode_prompt(full, ["a cat's 2 hats!"]))
        state["surprise.weight"] = torch.zeros(1)
        torch.save(state, str(d / "text_encoder" / "pytorch_model.bin"))
        with pytest.raises(RuntimeError, match="1 unexpected"):
            load_ldm("cpu", str(d), feature_upsample_res=32, text_encoder=True)
    finally:
        P.guess_arch = orig


# ---------------------------------------------------------------------------------------------------------------------
# C ABI, ledger
# ---------------------------------------------------------------------------------------------------------------------
def test_abi_argument_checks_without_a_gpu():
    from stablekeypoints_amd import _native as N
    lib = N.lib()                                                                           # dlopen works without a GPU
    assert lib.skp_abi_version() == N.ABI_VERSION >= 43
    assert lib.skp_text_attn_fwd_ok(1, 12, 77, 64, 2304) == 1
    assert lib.skp_text_attn_fwd_ok(1, 12, 77, 40, 2304) == 0                               # d = 40
    assert lib.skp_text_attn_fwd_ok(1, 12, 129, 64, 2304) == 0                              # N = 129
    assert lib.skp_text_attn_fwd_ok(1, 3, 77, 64, 190) == 0                                 # ld = 190: below H*d, no multiple of 4
    assert lib.skp_text_attn_fwd_ok(1, 3, 77, 64, 194) == 0 and lib.skp_text_attn_fwd_ok(1, 3, 77, 64, 196) == 1
    assert lib.skp_text_attn_fwd_ok(2, 3, 128, 32, 96) == 1 and lib.skp_text_attn_fwd_ok(0, 3, 77, 64, 192) == 0
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf) // 16 * 16 + 16                                               # a 16-byte aligned non-null address
    BADARG, RANGE = -1, -2
    f = lib.skp_text_attn_fwd_f32
    for args in ((None, p, p, p), (p, None, p, p), (p, p, None, p), (p, p, p, None)):
        assert f(*args, 1, 12, 77, 64, 768, 0.125, None) == BADARG
    assert f(p, p, p, p, 0, 12, 77, 64, 768, 0.125, None) == BADARG
    assert f(p, p, p, p, 1, 12, -1, 64, 768, 0.125, None) == BADARG
    assert f(p + 4, p, p, p, 1, 12, 77, 64, 768, 0.125, None) == BADARG                     # misaligned base
    assert f(p, p, p, p, 1, 12, 77, 40, 480, 0.125, None) == RANGE
    assert f(p, p, p, p, 1, 12, 129, 64, 768, 0.125, None) == RANGE
    assert f(p, p, p, p, 1, 3, 77, 64, 190, 0.125, None) == RANGE


def test_ledger_site_and_host_notes():
    from stablekeypoints_amd import ops, routes
    assert routes.ROUTES["text.attention"] == {"causal_fused": "hip", "lib_core": "library", "host": "host"}
    assert routes.kind("text.attention", "lib_core") == "library"
    assert ("text.attention", "lib_core") not in routes.DOCUMENTED_LIBRARY_ROUTES
    m = T.tower(96, 3, "gelu")
    before = routes.snapshot()
    m(T.prompt_ids())
    assert routes.delta(before) == {("text.attention", "host"): 2}                           # once per layer
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.text_attention(torch.zeros(1, 4, 192), None, None, 1, 1.0)
    assert ops.TEXT_ATTN_MODE == "auto"


def test_reference_error_is_meaningful_for_every_kernel_case():
    """err_fp32ref of every (family, shape) the GPU test runs is finite, and non-zero except where the output is exact in every
    precision: N = 1 (one key, weight 1) and `first_only` (the +100 key takes the whole weight: out = v[0] to the last bit in fp32
    and fp64 alike), whose bound is then the absolute 1e-7 alone."""
    for family in T.FAMILIES:
        for N in T.SIZES:
            for d in T.HEAD_DIMS:
                for B, H in T.BATCH_HEADS:
                    c = T.case(family, B, H, N, d)
                    e = c.err32["out"]
                    assert math.isfinite(e) and bool(torch.isfinite(c.ref64["out"]).all())
                    assert (e == 0) == (N == 1 or family == "first_only"), (family, N, d, B, H, e)
    # the own families do what they say: unmasked, every future key of diag_ramp outweighs the diagonal; key 0 tops first_only
    S = T.causal_logits(*(lambda c: (c.q, c.k, c.scale, c.H))(T.case("diag_ramp", 2, 3, 33, 64)))
    assert bool(((S[..., 1:] - S[..., :-1]).mean(dim=(0, 1, 2)) > 2).all()) and bool((S.argmax(-1) >= 28).all())
    S = T.causal_logits(*(lambda c: (c.q, c.k, c.scale, c.H))(T.case("first_only", 2, 3, 33, 64)))
    assert bool((S.argmax(-1) == 0).all()) and S[..., 0].min().item() > 90


# ---------------------------------------------------------------------------------------------------------------------
# sampling
# ---------------------------------------------------------------------------------------------------------------------
def test_uncond_prompt_on_the_host(tiny_pair):
    from stablekeypoints_amd import ptp_utils
    plain, pctrl, full, ctrl = tiny_pair
    emb = torch.randn(1, 77, 768, generator=torch.Generator().manual_seed(3))
    lat = torch.randn(1, 4, 8, 8, generator=torch.Generator().manual_seed(4))
    kw = dict(num_inference_steps=2, latent=lat, height=64, width=64)
    unc = ptp_utils.encode_prompt(full, [""])
    a, _ = ptp_utils.text2image_ldm_stable(full, emb, ctrl, uncond_prompt="", **kw)
    b, _ = ptp_utils.text2image_ldm_stable(full, emb, ctrl, uncond_embedding=unc, **kw)
    assert (a == b).all()
    c, _ = ptp_utils.text2image_ldm_stable(full, emb, ctrl, **kw)
    d, _ = ptp_utils.text2image_ldm_stable(plain, emb, pctrl, **kw)
    assert (c == d).all()
    with pytest.raises(ValueError, match="mutually exclusive"):
        ptp_utils.text2image_ldm_stable(full, emb, ctrl, uncond_prompt="", uncond_embedding=unc, **kw)
    with pytest.raises(RuntimeError, match="text_encoder=True"):
        ptp_utils.text2image_ldm_stable(plain, emb, pctrl, uncond_prompt="", **kw)
    with pytest.raises(RuntimeError, match="text_encoder=True"):
        ptp_utils.encode_prompt(plain, [""])
