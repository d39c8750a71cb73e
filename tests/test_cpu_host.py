"""CPU tests (-m "not gpu") of the host side: C-ABI library loads and exports every declared symbol, the
PrithviSeg state_dict / checkpoint contract, config surface, and that nothing computes without the GPU."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "instageo-e2e-geospatial-ml_amd")


@pytest.fixture(scope="session")
def built_lib():
    from instageo_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(PKG, "csrc"), "-j4"], check=True)
    return _lib


def test_library_exports_every_declared_symbol(built_lib):
    lib = built_lib.load()
    names = built_lib.declared_symbols()
    assert len(names) >= 30
    header = open(built_lib.HEADER_PATH).read()
    for n in re.findall(r"\b(ig_\w+)\s*\(", header):
        assert hasattr(lib, n), n
    assert lib.ig_version() >= 100
    assert built_lib.last_error() == "" or isinstance(built_lib.last_error(), str)


def test_argument_validation_without_gpu(built_lib):
    """IG_REQUIRE rejects bad arguments before any launch, so these calls are safe on a CPU-only box."""
    lib = built_lib.load()
    rc = lib.ig_linear_fwd(None, None, None, None, None, None, None, None, None, 8, 8, 8, 0, None)
    assert rc == -1 and "null pointer" in built_lib.last_error()
    one = ctypes.c_void_p(16)
    rc = lib.ig_linear_fwd(one, None, one, None, None, one, None, None, None, 8, 12, 12, 0, None)
    assert rc == -1 and "multiples of 8" in built_lib.last_error()
    rc = lib.ig_attention_fwd(one, None, one, None, None, 1, 8, 1, 32, None)
    assert rc == -1 and "head_dim" in built_lib.last_error()
    with pytest.raises(built_lib.HipLibraryError):
        built_lib.call("ig_ce_loss", one, one, 7, None, -1, None, None, None, None, None, 1, 4, 99, None)


def test_ops_refuse_cpu_tensors(built_lib):
    from instageo_amd import ops

    x = torch.zeros(8, 8, dtype=torch.bfloat16)
    with pytest.raises(built_lib.HipLibraryError):
        ops.linear_fwd(ops.BT(x), ops.BT(x), None, ops.BT(x), 8, 8, 8)


def test_product_never_imports_oracle():
    for dirpath, _, files in os.walk(os.path.join(PKG, "instageo_amd")):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(dirpath, f)).read()
                assert "oracle" not in src.replace("# oracle", ""), f"{f} mentions the oracle"


@pytest.mark.parametrize("variant,T,ncls", [("prithvi_eo_tiny", 1, 2), ("prithvi_eo_tiny", 3, 13), ("prithvi_eo_v1_100", 1, 2)])
def test_prithviseg_state_dict_contract(variant, T, ncls):
    from instageo_amd.model import PrithviSeg
    from oracle import prithvi_oracle as O

    net = PrithviSeg(temporal_step=T, num_classes=ncls, load_pretrained_weights=False, freeze_backbone=False, variant=variant, device="cpu")
    cfg = O.make_config(variant, T, ncls)
    want = O.state_dict_shapes(cfg)  # verified equal to the reference's keys/shapes by oracle/gen_golden.py
    got = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    assert got == want and list(got) == list(want)
    sd = O.make_state_dict(cfg, seed=7)
    net.load_state_dict(sd, strict=True)
    back = net.state_dict()
    assert all(torch.equal(back[k], sd[k]) for k in sd)
    # conv weights are stored [Cout][9][Cin] but exposed with the PyTorch shapes
    e = net.store.entries["segmentation_head.1.2.weight"]
    w = sd["segmentation_head.1.2.weight"]
    assert torch.equal(net.store.flat[e.offset : e.offset + e.numel].view(w.shape[0], 9, w.shape[1]), w.permute(0, 2, 3, 1).reshape(w.shape[0], 9, -1))
    e = net.store.entries["segmentation_head.1.0.weight"]
    w = sd["segmentation_head.1.0.weight"]
    assert torch.equal(net.store.flat[e.offset : e.offset + e.numel].view(w.shape[1], 9, w.shape[0]), w.permute(1, 2, 3, 0).reshape(w.shape[1], 9, -1))
    bad = dict(sd)
    bad.pop("segmentation_head.5.bias")
    with pytest.raises(RuntimeError):
        net.load_state_dict(bad, strict=True)
    assert hasattr(net, "prithvi_encoder") and hasattr(net, "segmentation_head") and net.model_args["num_frames"] == T


def test_tl_variant_carries_the_unused_coordinate_encoder_scales():
    """prithvi_eo_v2_300_tl (model.py:147-153): the reference builds Temporal/LocationEncoder but PrithviViT.forward never calls
    them -- same arithmetic as prithvi_eo_v2_300 plus two (1,) ``scale`` parameters that get no gradient and are never stepped.
    Key order / shapes / zero gradients were checked against the imported reference in the build container;
    the 600M variants (patch 14, head_dim 80, 5x5 / 7x7 head kernels) still raise."""
    from instageo_amd.model import PrithviSeg
    from oracle import prithvi_oracle as O

    net = PrithviSeg(temporal_step=1, num_classes=2, load_pretrained_weights=False, freeze_backbone=False,
                     variant="prithvi_eo_v2_300_tl", depth=1, device="cpu")
    cfg = O.make_config("prithvi_eo_v2_300_tl", 1, 2, 224, 1)
    want = O.state_dict_shapes(cfg)
    got = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    assert got == want and list(got) == list(want)
    keys = list(got)
    i = keys.index("prithvi_encoder.patch_embed.proj.bias")
    assert keys[i + 1 : i + 3] == ["prithvi_encoder.temporal_embed_enc.scale", "prithvi_encoder.location_embed_enc.scale"]
    sd = net.state_dict()
    assert float(sd["prithvi_encoder.temporal_embed_enc.scale"]) == pytest.approx(0.1) and net.prithvi_encoder.location_embed_enc.scale.requires_grad
    assert "prithvi_encoder.temporal_embed_enc.scale" not in net.store.entries  # outside the flat buffer: AdamW never touches it
    new = O.make_state_dict(cfg, seed=3)
    net.load_state_dict(new, strict=True)
    assert torch.equal(net.state_dict()["prithvi_encoder.location_embed_enc.scale"], new["prithvi_encoder.location_embed_enc.scale"])
    # the 600M family (model.py:154-177): D = 1280, 16 heads of 80, patch 14, head kernels [5, 5, 5, 7] -- same key / shape contract
    for v in ("prithvi_eo_v2_600", "prithvi_eo_v2_600_tl"):
        n6 = PrithviSeg(load_pretrained_weights=False, variant=v, depth=1, device="cpu")
        c6 = O.make_config(v, 1, 2, 224, 1)
        want6 = O.state_dict_shapes(c6)
        got6 = {k: tuple(t.shape) for k, t in n6.state_dict().items()}
        assert got6 == want6 and list(got6) == list(want6)
        assert got6["segmentation_head.0.2.weight"] == (640, 640, 5, 5) and got6["segmentation_head.3.2.weight"] == (80, 80, 7, 7)
        assert got6["prithvi_encoder.patch_embed.proj.weight"] == (1280, 6, 1, 14, 14) and got6["prithvi_encoder.pos_embed"] == (1, 257, 1280)
        assert n6.cfg.head_sizes == [(16, 32, 30), (30, 60, 58), (58, 116, 114), (114, 228, 224)] and n6.cfg.out_size == 224
        n6.load_state_dict(O.make_state_dict(c6, seed=5), strict=True)


def test_reference_init_statistics():
    from instageo_amd.model import PrithviSeg

    torch.manual_seed(0)
    net = PrithviSeg(temporal_step=1, num_classes=2, load_pretrained_weights=False, freeze_backbone=True, variant="prithvi_eo_tiny", device="cpu")
    sd = net.state_dict()
    assert torch.all(sd["prithvi_encoder.pos_embed"][0, 0] == 0)
    assert torch.all(sd["prithvi_encoder.blocks.0.norm1.weight"] == 1) and torch.all(sd["prithvi_encoder.blocks.0.attn.qkv.bias"] == 0)
    w = sd["prithvi_encoder.blocks.0.mlp.fc1.weight"]
    bound = (6.0 / (w.shape[0] + w.shape[1])) ** 0.5  # xavier_uniform (pritvhi.py:140-143)
    assert w.abs().max() <= bound + 1e-6 and w.abs().max() > 0.9 * bound
    assert abs(sd["prithvi_encoder.cls_token"].std().item() - 0.02) < 0.005
    assert all(not p.requires_grad for p in net.prithvi_encoder.parameters())  # freeze_backbone (model.py:341-343)
    assert all(p.requires_grad for p in net.segmentation_head.parameters())


def test_checkpoint_layout_and_mae_checkpoint_filter(tmp_path):
    from instageo_amd.model import load_prithvi_checkpoint
    from instageo_amd.segmentation import PrithviSegmentationModule

    mod = PrithviSegmentationModule(freeze_backbone=False, load_pretrained_weights=False, num_classes=2, model_name="prithvi_eo_tiny",
                                    class_weights=[1, 3], ignore_index=-1, device="cpu")
    ck = mod.checkpoint_state_dict()
    assert "criterion.weight" in ck and all(k.startswith("net.") or k == "criterion.weight" for k in ck)
    torch.save({"state_dict": ck}, tmp_path / "instageo_best_checkpoint.ckpt")
    mod2 = PrithviSegmentationModule(freeze_backbone=False, load_pretrained_weights=False, num_classes=2, model_name="prithvi_eo_tiny",
                                     class_weights=[1, 3], ignore_index=-1, device="cpu")
    mod2.load_checkpoint_state_dict(torch.load(tmp_path / "instageo_best_checkpoint.ckpt")["state_dict"])
    assert all(torch.equal(a, b) for a, b in zip(mod.net.state_dict().values(), mod2.net.state_dict().values()))
    # a Prithvi MAE checkpoint: encoder.* prefix, decoder keys, mask_token, foreign pos_embed (utils.py:271-315)
    enc = {k[len("prithvi_encoder."):]: v.clone() for k, v in mod.net.state_dict().items() if k.startswith("prithvi_encoder.")}
    mae = {"encoder." + k: (torch.randn_like(v) if v.is_floating_point() else v) for k, v in enc.items()}
    mae["encoder.pos_embed"] = torch.randn(1, 5, 256)
    mae["decoder.blocks.0.norm1.weight"] = torch.zeros(3)
    mae["mask_token"] = torch.zeros(1, 1, 128)
    pos_before = mod2.net.state_dict()["prithvi_encoder.pos_embed"].clone()
    load_prithvi_checkpoint(mod2.net, mae)
    sd2 = mod2.net.state_dict()
    assert torch.equal(sd2["prithvi_encoder.pos_embed"], pos_before)  # model's own fixed table is kept
    assert torch.equal(sd2["prithvi_encoder.blocks.1.mlp.fc1.weight"], mae["encoder.blocks.1.mlp.fc1.weight"])


def test_unsupported_and_pretrained_paths_fail_loudly():
    from instageo_amd.model import PrithviSeg

    with pytest.raises(KeyError):
        PrithviSeg(variant="prithvi_eo_v3_900", load_pretrained_weights=False, device="cpu")
    with pytest.raises(RuntimeError):
        PrithviSeg(variant="prithvi_eo_tiny", load_pretrained_weights=True, device="cpu")
    net = PrithviSeg(variant="prithvi_eo_tiny", load_pretrained_weights=False, device="cpu")
    from instageo_amd._lib import HipLibraryError

    with pytest.raises(HipLibraryError):
        net(torch.zeros(1, 6, 1, 224, 224))
    with pytest.raises(TypeError):
        net.double()


def test_metrics_host_arithmetic_matches_oracle():
    from instageo_amd.metrics import metrics_from_matrix
    from oracle import prithvi_oracle as O

    rng = np.random.default_rng(3)
    cm = rng.integers(0, 50, size=(13, 13))
    cm[5] = 0
    cm[:, 5] = 0  # an absent class -> zero denominators
    a, b = metrics_from_matrix(cm), O.confusion_metrics(cm)
    for k in a:
        assert np.allclose(a[k], b[k], atol=1e-12), k


def test_config_surface():
    from instageo_amd.config import DEFAULTS, check_required_flags, load_config

    # every top-level / nested key of the reference's config.yaml (SURVEY.md 8b "CLI surface to keep")
    assert {"root_dir", "valid_filepath", "train_filepath", "test_filepath", "checkpoint_path", "mode", "is_reg_task", "train", "model",
            "dataloader", "test"} <= set(DEFAULTS)
    assert {"learning_rate", "num_epochs", "batch_size", "class_weights", "ignore_index", "weight_decay", "scheduler", "distillation",
            "teacher_ckpt_path"} <= set(DEFAULTS["train"])
    assert {"bands", "mean", "std", "img_size", "temporal_dim", "replace_label", "reduce_to_zero", "no_data_value", "constant_multiplier",
            "max_pixel_value", "num_workers", "augmentations"} <= set(DEFAULTS["dataloader"])
    assert {"img_size", "crop_size", "stride", "mask_cloud"} <= set(DEFAULTS["test"])
    c = load_config("sen1floods11", ["train.batch_size=4", "mode=eval", "+neptune_experiment_id=abc", "model.weight_clip_range=[-1,1]"])
    assert c["train"]["batch_size"] == 4 and c["train"]["class_weights"] == [1, 3] and c["test"]["img_size"] == 512
    assert c["model"]["model_name"] == "prithvi_eo_v1_100" and c["neptune_experiment_id"] == "abc" and c["model"]["weight_clip_range"] == [-1, 1]
    m = load_config("multitemporal_crop_classification")
    assert m["dataloader"]["temporal_dim"] == 3 and m["model"]["num_classes"] == 13 and len(m["train"]["class_weights"]) == 13
    with pytest.raises(KeyError):
        load_config("config", ["train.nonexistent=1"])
    with pytest.raises(KeyError):
        load_config("nope")
    with pytest.raises(RuntimeError):
        check_required_flags(["root_dir"], {"root_dir": "None"})  # the *string* "None" counts as missing
    check_required_flags(["root_dir"], {"root_dir": "/data"})


def test_torch_library_ops_are_registered_from_the_header():
    """SURVEY.md 8b / north_star: the hot path sits behind PyTorch custom ops.  Every C-ABI entry point that takes device
    pointers is a dispatcher-visible ``instageo_mi355x::`` op whose schema is generated from include/instageo_hip.h
    (non-const pointers = mutated arguments), with a fake implementation; there is no CPU kernel."""
    import torch
    from torch._subclasses.fake_tensor import FakeTensorMode

    from instageo_amd import _lib, torch_ops

    ops_ = torch_ops.register()
    assert torch_ops.register() is ops_  # idempotent
    protos = torch_ops.parse_prototypes()
    tensor_entries = [n for n, ps in protos.items() if n not in torch_ops._SKIP and any("*" in t for t, pn in ps if pn != "stream")]
    assert sorted(ops_) == sorted(n[3:] for n in tensor_entries) and len(ops_) >= 40
    assert set(protos) <= set(_lib.declared_symbols())
    sch = str(torch.ops.instageo_mi355x.linear_fwd.default._schema)
    assert "Tensor? x_hi" in sch and "Tensor(a!)? y_hi" in sch and sch.endswith("int M, int N, int K, int act) -> ()")
    assert "Tensor(a!)? dw" in str(torch.ops.instageo_mi355x.linear_wgrad.default._schema)
    with FakeTensorMode():
        x = torch.empty(64, 32, dtype=torch.bfloat16, device="cuda")
        w = torch.empty(16, 32, dtype=torch.bfloat16, device="cuda")
        y, d = torch.ops.instageo_mi355x.linear(x, w, None, 1)
        assert y.shape == (64, 16) and d.shape == (64, 16) and y.dtype == torch.bfloat16
        assert torch.ops.instageo_mi355x.linear_fwd(x, None, w, None, None, y, None, None, None, 64, 16, 32, 0) is None
        a, m, r = torch.ops.instageo_mi355x.layer_norm(torch.empty(64, 32, device="cuda"), torch.empty(32, device="cuda"), torch.empty(32, device="cuda"), 1e-5)
        assert a.dtype == torch.bfloat16 and m.shape == (64,) and r.shape == (64,)
    import pytest

    with pytest.raises(NotImplementedError):  # no CPU backend
        torch.ops.instageo_mi355x.linear(torch.empty(4, 8, dtype=torch.bfloat16), torch.empty(8, 8, dtype=torch.bfloat16), None, 0)


@pytest.mark.parametrize("variant", ["prithvi_eo_v1_100", "prithvi_eo_v2_300"])
def test_block_gradient_range_tables_partition_the_flat_buffer(variant):
    """Host logic behind the deterministic folds and the fresh-step zeroing (model.py): the "small ranges" of a Block are exactly its
    flat range minus the four weight matrices the grouped weight-gradient kernel writes -- nothing left out, nothing twice -- and the
    notification ranges of a backward pass tile [0, total)."""
    from instageo_amd.model import PrithviSeg

    net = PrithviSeg(variant=variant, load_pretrained_weights=False, device="cpu")
    eng, ent = net.engine, net.engine.store.entries
    L = eng.cfg.depth
    e = "prithvi_encoder."
    starts = [ent[f"{e}blocks.{i}.norm1.weight"].offset for i in range(L)] + [ent[e + "norm.weight"].offset]
    for i in (0, L // 2, L - 1):
        lo, hi = starts[i], starts[i + 1]
        small = eng._block_small_ranges(i, lo, hi)
        big = sorted((ent[f"{e}blocks.{i}.{n}"].offset, ent[f"{e}blocks.{i}.{n}"].offset + ent[f"{e}blocks.{i}.{n}"].numel) for n in eng._BLOCK_WEIGHTS)
        pieces = sorted(small + big)
        assert pieces[0][0] == lo and pieces[-1][1] == hi
        assert all(a[1] == b[0] for a, b in zip(pieces, pieces[1:])), "gap or overlap inside a Block"
        assert all(b > a for a, b in small)
        D = eng.cfg.embed_dim
        assert sum(b - a for a, b in small) == 13 * D  # 2 LayerNorms (4 D) + biases of qkv (3 D), proj (D), fc1 (4 D), fc2 (D)
    # the notification ranges of SegEngine.backward: head | final norm | blocks L-1 .. 0 | cls token + patch embedding
    head0 = ent["segmentation_head.0.0.weight"].offset
    tiles = [(head0, eng.store.total), (starts[L], head0)] + [(starts[i], starts[i + 1]) for i in range(L - 1, -1, -1)]
    tiles.append((ent[e + "cls_token"].offset, starts[0]))
    tiles.sort()
    assert tiles[0][0] == 0 and tiles[-1][1] == eng.store.total and all(a[1] == b[0] for a, b in zip(tiles, tiles[1:]))


def test_whole_network_custom_op_is_registered_with_a_fake_implementation():
    """``instageo_mi355x::prithvi_seg`` (torch_ops.py): schema, fake (meta) shapes of logits / features, and no CPU kernel --
    ``PrithviSeg.forward`` dispatches through it (checked on the GPU by tests/test_gpu_model.py)."""
    from torch._subclasses.fake_tensor import FakeTensorMode

    from instageo_amd import torch_ops
    from instageo_amd.model import PrithviSeg

    torch_ops.register()
    op = torch.ops.instageo_mi355x.prithvi_seg
    assert "Tensor[] params" in str(op.default._schema) and "int handle" in str(op.default._schema)
    net = PrithviSeg(variant="prithvi_eo_tiny", temporal_step=3, num_classes=13, load_pretrained_weights=False, device="cpu")
    with FakeTensorMode():
        img = torch.empty(2, 6, 3, 224, 224)
        ps = [torch.empty(p.shape) for _, p in net._flat_params()]
        logits, feats, gen = op(img, ps, net._handle, False, False, True)
        assert logits.shape == (2, 13, 224, 224) and feats.shape == (2, 256 * 3, 14, 14)
        assert gen.shape == (1,) and gen.dtype == torch.int64 and gen.device.type == "cpu"  # the forward generation travels as an op OUTPUT
        grads = torch.ops.instageo_mi355x.prithvi_seg_backward(logits, ps, net._handle, gen)
        assert len(grads) == len(ps)
    with pytest.raises(NotImplementedError):  # no CPU backend
        op(torch.zeros(1, 6, 3, 224, 224), [p.detach() for _, p in net._flat_params()], net._handle, False, False, False)
    handle = net._handle
    del net
    import gc

    gc.collect()
    with pytest.raises(RuntimeError):
        from instageo_amd.model import network_of

        network_of(handle)


def test_m0_is_only_written_by_the_lds_dma_helpers():
    """gemm8.hip / gemm8w.hip / conv8.hip / gemm4.hip set M0 (the LDS destination of an LDS-DMA) without saving or restoring it (the asm statements
    declare the clobber).  That is sound and free only while hipcc keeps nothing of its own in M0 in those kernels: compile each file to gfx950
    assembly (no GPU needed) and check that every M0 reference is one of the helpers' `s_mov_b32 m0, sN` -- or, in the generated K-loops of
    gemm4.hip, gemm8w.hip's gemm4w_kernel and conv8.hip's conv4_kernel, `s_add_u32 m0, sN, imm` -- no read of M0, no other writer."""
    import re
    import shutil
    import subprocess
    import tempfile

    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "instageo-e2e-geospatial-ml_amd", "csrc")
    with tempfile.TemporaryDirectory() as tmp:
        if not os.path.exists(os.path.join(csrc, "gemm4_gen.inc")):  # normally written by the Makefile
            subprocess.run([sys.executable, os.path.join(csrc, "gen_gemm4.py"), os.path.join(csrc, "gemm4_gen.inc")], check=True)
        for name in ("gemm8", "gemm8w", "conv8", "gemm4"):
            out = os.path.join(tmp, name + ".s")
            subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-I" + os.path.join(root, "include"), "-DIG_HEADER_STAMP=0", "-S",
                            "--cuda-device-only", os.path.join(csrc, name + ".hip"), "-o", out], check=True, capture_output=True)
            refs = [ln.strip() for ln in open(out) if re.search(r"\bm0\b", ln) and not ln.lstrip().startswith(";")]
            assert refs, name
            bad = [ln for ln in refs if not re.fullmatch(r"s_mov_b32 m0, s\d+", ln) and not (name in ("gemm4", "gemm8w", "conv8") and re.fullmatch(r"s_add_u32 m0, s\d+, (0x)?[0-9a-f]+", ln))]
            assert not bad, (name, bad[:5])


# ---- csrc/gen_gemm4.py: helpers of the generator tests below
_G4_MF = "v_mfma_f32_16x16x32_bf16"
_G4_MF_OPERANDS = _G4_MF + r" a\[\d+:\d+\], v\[(\d+):\d+\], v\[(\d+):\d+\]"


def _g4_run(out, *args):
    """run the generator the way the Makefile does: output path, then key=value arguments"""
    return subprocess.run([sys.executable, os.path.join(PKG, "csrc", "gen_gemm4.py"), str(out), *args], capture_output=True, text=True)


def _g4_generate(tmp_path, *args):
    out = tmp_path / "g4.inc"
    r = _g4_run(out, *args)
    assert r.returncode == 0, r.stderr
    return out.read_text()


def _g4_macros(text):
    """macro name -> body (everything behind the name, continuation lines included); "readout" -> the C++ helpers behind the last macro"""
    m = dict(re.findall(r"^#define (G4\w+)((?:.*\\\n)*.*)$", text, re.M))
    m["readout"] = text[text.index("__device__"):]
    return m


def _g4_block(text, name):
    """the instructions of an asm macro"""
    return re.findall(r'"([^"]*?)\\n\\t"', _g4_macros(text)[name])


def _g4_check_regs(ins, clob):
    """every VGPR / SGPR the instructions name lies inside the clobber list, which declares all AGPRs, M0, SCC and memory; returns the VGPRs"""
    cv = {int(x) for x in re.findall(r'"v(\d+)"', clob)}
    cs = {int(x) for x in re.findall(r'"s(\d+)"', clob)}
    assert {int(x) for x in re.findall(r'"a(\d+)"', clob)} == set(range(256)) and '"m0"' in clob and '"scc"' in clob and '"memory"' in clob
    for i in ins:
        body = re.sub(r"%\[[a-z0-9_]+\]", "", i)
        for lo, hi in re.findall(r"\bv\[(\d+):(\d+)\]", body):
            assert set(range(int(lo), int(hi) + 1)) <= cv, i
        for r in re.findall(r"\bv(\d+)\b", body):
            assert int(r) in cv, i
        for lo, hi in re.findall(r"\bs\[(\d+):(\d+)\]", body):
            assert set(range(int(lo), int(hi) + 1)) <= cs, i
        for r in re.findall(r"\bs(\d+)\b", body):
            assert int(r) in cs, i
    return cv


def _g4_check_m0_spacing(ins, prefix):
    """every LDS-DMA issue (mnemonic prefix) has its own M0 write two instructions earlier and something else in between (the wait state M0
    needs); returns the issues' positions"""
    dma = [k for k, i in enumerate(ins) if i.startswith(prefix)]
    for k in dma:
        assert ins[k - 2].startswith("s_add_u32 m0, ") and not ins[k - 1].startswith(("s_add_u32 m0", "buffer_load", "global_load")), ins[k - 2:k + 1]
    return dma


def _g4_halves(ins):
    """the stream split behind the waits that end a half"""
    out, half = [], []
    for i in ins:
        half.append(i)
        if i == "s_waitcnt lgkmcnt(0)":
            out.append(half)
            half = []
    return out


def _g4_products(ins, per):
    """the stream from the first to the last MFMA of every run of `per` MFMAs"""
    mfk = [k for k, i in enumerate(ins) if i.startswith(_G4_MF)]
    return [ins[mfk[b]:mfk[b + per - 1] + 1] for b in range(0, len(mfk), per)]


def _g4_check_reads_spare_consumed_sets(groups, rd):
    """in every group (a half or a product) no read (mnemonic rd) writes a fragment block that the group's own MFMAs consume"""
    for n, g in enumerate(groups):
        used = set()
        for i in g:
            m = re.match(_G4_MF_OPERANDS, i)
            if m:
                used |= {int(m.group(1)), int(m.group(2))}
        for i in g:
            m = re.match(rd + r" v\[(\d+):", i)
            if m:
                assert int(m.group(1)) // 4 * 4 not in used, (i, n)


def test_gemm4w_generator_emits_a_consistent_instruction_stream(tmp_path):
    """The weight-gradient forms of csrc/gen_gemm4.py (gemm4w_kernel in gemm8w.hip: plain, short-segment and paired blocks).  Structural
    invariants of the generated text:
    * plain segment block: 6 iterations of 128 MFMAs (first / middle / last pair), only the first 64 start from 0; 64 transposed fragment reads
      per iteration (+ 32 at entry); 16 buffer LDS-DMA issues per iteration, each two instructions behind its own M0 write; one vmcnt(8) + one
      barrier per iteration; the descriptors are re-pointed at the next segment exactly once, in front of the last pair; the short block is the
      first-and-last pair alone;
    * paired block: 6 iterations of 192 MFMAs in three products, 64 reads per iteration (+ 48 at entry), 16 DMA issues, and no product's reads
      write a quarter set its own MFMAs consume;
    * every named register lies inside the clobber list; the clobbered VGPR range leaves the low registers to the compiler."""
    text = _g4_generate(tmp_path)

    def check_dma(ins, n):
        dma = _g4_check_m0_spacing(ins, "buffer_load_dwordx4")
        assert len(dma) == n and all(ins[k].endswith("offen lds") for k in dma)

    MF, RD = _G4_MF, "ds_read_b64_tr_b16"
    seg, short, pro = _g4_block(text, "G4W_ASM_SEG"), _g4_block(text, "G4W_ASM_SEG_SHORT"), _g4_block(text, "G4W_ASM_PROLOGUE")
    for ins, iters in ((seg, 6), (short, 2)):
        mf = [i for i in ins if i.startswith(MF)]
        assert len(mf) == iters * 128 and all(i.endswith(", 0") for i in mf[:64]) and sum(1 for i in mf if i.endswith(", 0")) == 64
        for it in range(iters):
            dst = [int(re.match(MF + r" a\[(\d+):", i).group(1)) for i in mf[it * 128:(it + 1) * 128]]
            assert sorted(dst) == sorted([4 * b for b in range(64)] * 2)
        assert sum(1 for i in ins if i.startswith(RD)) == 32 + iters * 64
        check_dma(ins, iters * 16)
        assert sum(1 for i in ins if i == "s_waitcnt vmcnt(8)") == iters and sum(1 for i in ins if i == "s_barrier") == iters + 1
        assert sum(1 for i in ins if i == "s_waitcnt vmcnt(0)") == 1
        # descriptors: set up once at entry, re-pointed once (the next segment) in front of the last pair
        flags = [k for k, i in enumerate(ins) if i.endswith("0x00020000")]
        assert len(flags) == 4
        mfk = [k for k, i in enumerate(ins) if i.startswith(MF)]
        assert flags[1] < mfk[0] and mfk[(iters - 2) * 128 - 1] < flags[2] < flags[3] < mfk[(iters - 2) * 128] if iters > 2 else flags[3] < mfk[0]
    check_dma(pro, 32)
    cv = _g4_check_regs(seg + short + pro, _g4_macros(text)["G4W_CLOBBERS"])
    assert min(cv) >= 48  # the compiler keeps v0 .. v47 at least
    _g4_check_reads_spare_consumed_sets(_g4_halves(seg), RD)  # a half's reads never write the fragment set its own MFMAs consume
    # ---- paired form
    pseg, ppro = _g4_block(text, "G4WP_ASM_SEG"), _g4_block(text, "G4WP_ASM_PROLOGUE")
    pmf = [k for k, i in enumerate(pseg) if i.startswith(MF)]
    assert len(pmf) == 6 * 192 and all(pseg[k].endswith(", 0") for k in pmf[:64]) and sum(1 for k in pmf if pseg[k].endswith(", 0")) == 64
    assert sum(1 for i in pseg if i.startswith(RD)) == 48 + 6 * 64
    check_dma(pseg, 6 * 16)
    check_dma(ppro, 32)
    assert sum(1 for i in pseg if i == "s_waitcnt vmcnt(8)") == 6 and sum(1 for i in pseg if i == "s_barrier") == 7
    pcv = _g4_check_regs(pseg + ppro, _g4_macros(text)["G4WP_CLOBBERS"])
    assert min(pcv) >= 32
    _g4_check_reads_spare_consumed_sets(_g4_products(pseg, 64), RD)


def test_conv4_generator_emits_a_consistent_instruction_stream(tmp_path):
    """The convolution form of csrc/gen_gemm4.py (conv4_kernel in conv8.hip: 256 x 192 tile, gathered A pieces).  Per iteration: 16 NI MFMAs on
    8 x NI accumulator blocks (NI = 6: 256 x 192 tile, 3: 256 x 96), 2 (8 + NI) fragment reads, 8 gathered A pieces -- each `buffer_load ... offen lds` preceded by its own M0 write and by the
    three instructions that build its offset from the row offset, the row's inverted tap mask and this K-tile's table entry -- and NI plain B
    pieces; one table read per iteration, behind the decode of the previous entry; the last pair takes the NEXT tile's rows; every named
    register lies inside the clobber list."""
    text = _g4_generate(tmp_path)
    for NI in (6, 3):
        _check_conv4_blocks(text, NI)
    # ---- the paired split form (256 x 192 tile): three products of 48 MFMAs per 32-element K-tile on five quarter sets
    pt = _g4_block(text, "G4CP6_ASM_TILE")
    pmf = [k for k, i in enumerate(pt) if i.startswith(_G4_MF)]
    assert len(pmf) == 6 * 3 * 48 and all(pt[k].endswith(", 0") for k in pmf[:48]) and sum(1 for k in pmf if pt[k].endswith(", 0")) == 48
    assert sum(1 for i in pt if i.startswith("ds_read_b128")) == (8 + 8 + 6) + 6 * (6 + 8 + 6 + 8)
    assert sum(1 for i in pt if i.startswith("buffer_load_dwordx4")) == 6 * 8 and sum(1 for i in pt if i.startswith("global_load_lds_dwordx4")) == 6 * 6
    assert sum(1 for i in pt if i.startswith("ds_read_b32")) == 7 and sum(1 for i in pt if i == "s_barrier") == 7
    _g4_check_regs(pt, _g4_macros(text)["G4CP6_CLOBBERS"])
    _g4_check_reads_spare_consumed_sets(_g4_products(pt, 48), "ds_read_b128")  # a product's reads never write a quarter set its own MFMAs consume


def _check_conv4_blocks(text, NI):
    tile, pro = _g4_block(text, "G4C%d_ASM_TILE" % NI), _g4_block(text, "G4C%d_ASM_PROLOGUE" % NI)
    MF = _G4_MF
    mf = [i for i in tile if i.startswith(MF)]
    H = 8 * NI
    assert len(mf) == 6 * 2 * H and all(i.endswith(", 0") for i in mf[:H]) and sum(1 for i in mf if i.endswith(", 0")) == H
    for it in range(6):
        dst = sorted(int(re.match(MF + r" a\[(\d+):", i).group(1)) for i in mf[it * 2 * H:(it + 1) * 2 * H])
        assert dst == sorted([(mi * 8 + ni) * 4 for mi in range(8) for ni in range(NI)] * 2)
    assert sum(1 for i in tile if i.startswith("ds_read_b128")) == (8 + NI) + 6 * 2 * (8 + NI)
    assert sum(1 for i in tile if i.startswith("ds_read_b32")) == 1 + 6 and sum(1 for i in pro if i.startswith("ds_read_b32")) == 2
    ga = _g4_check_m0_spacing(tile, "buffer_load_dwordx4")
    gb = _g4_check_m0_spacing(tile, "global_load_lds_dwordx4")
    assert len(ga) == 6 * 8 and len(gb) == 6 * NI
    for n, k in enumerate(ga):  # the piece's offset register is written by bfe -> lshl_add -> add, in that order, before the issue
        reg = re.match(r"buffer_load_dwordx4 (v\d+),", tile[k]).group(1)
        ops3 = [i for i in tile[:k] if re.match(r"v_(bfe_u32|lshl_add_u32|add_u32) " + reg + ",", i)][-3:]
        assert [o.split()[0] for o in ops3] == ["v_bfe_u32", "v_lshl_add_u32", "v_add_u32"], (reg, ops3)
        nxt = n >= 4 * 8  # the last pair gathers the next tile's rows
        assert ("%[imn" in ops3[0]) == nxt and ("%[ron" in ops3[2]) == nxt, ops3
    assert sum(1 for i in tile if i == "s_waitcnt vmcnt(8)") == 6 and sum(1 for i in tile if i == "s_barrier") == 7
    _g4_check_regs(tile + pro, _g4_macros(text)["G4C%d_CLOBBERS" % NI])


def test_split_tensors_are_one_allocation_with_lo_above_hi():
    """ops.BT allocates hi and lo of a split tensor as ONE block, lo a fixed multiple of 256 bytes above hi, and slices taken at the same
    position keep that distance: the paired split-mode kernels (gemm8.hip / conv8.hip NSEG = 2) carry it in the lo lanes' 32-bit offsets."""
    import torch
    from instageo_amd.ops import BT

    for shape in [(7,), (5, 3), (1000, 768), (2, 3, 5, 48)]:
        for make in (BT.empty, BT.zeros):
            t = make(shape, True, "cpu")
            assert t.hi.shape == torch.Size(shape) and t.lo.shape == t.hi.shape and t.hi.is_contiguous() and t.lo.is_contiguous()
            d = t.lo.data_ptr() - t.hi.data_ptr()
            assert d >= t.hi.numel() * 2 and d % 256 == 0
            assert t.hi.untyped_storage().data_ptr() == t.lo.untyped_storage().data_ptr()
            flat = BT(t.hi.reshape(-1), t.lo.reshape(-1))
            assert flat.lo[3:].data_ptr() - flat.hi[3:].data_ptr() == d
        z = BT.zeros(shape, True, "cpu")
        assert not z.hi.any() and not z.lo.any()
        z.hi.fill_(1)
        assert not z.lo.any()  # the halves do not overlap
    assert BT.empty((4, 4), False, "cpu").lo is None


def test_operand_copy_reads_refuse_an_in_flight_all_gather():
    """Data parallel, deferred all-gather (distributed.ShardedGradSync, IG_DP_DEFER=1): the bf16 operand copy above the lowest pending bucket
    is being written by RCCL.  ``ParamStore.w`` -- the only accessor of operand views -- raises for a parameter at or above that offset
    (the ordering used to rest on every reader remembering to call ``wait_params``); below it, and with nothing pending, it does not."""
    from instageo_amd.model import PrithviSeg

    net = PrithviSeg(variant="prithvi_eo_tiny", temporal_step=1, num_classes=2, load_pretrained_weights=False, device="cpu")
    st = net.store
    names = list(st.entries)
    first, last = names[0], names[-1]
    boundary = st.entries[last].offset
    st.pending_from = lambda: boundary
    with pytest.raises(RuntimeError, match="still in flight"):
        st.w(last)
    st.shadow = type("S", (), {"hi": st.flat.to(torch.bfloat16), "lo": None})()  # a stand-in operand copy (the real one is made by a HIP kernel)
    assert st.w(first).hi.numel() == st.entries[first].numel  # below the pending bucket: readable
    st.pending_from = lambda: None
    assert st.w(last).hi.numel() == st.entries[last].numel


def test_gemm4_generator_emits_a_consistent_instruction_stream(tmp_path):
    """csrc/gen_gemm4.py writes the hand-scheduled K-loop of gemm4.hip (one inline-asm block per tile, registers assigned by hand).  Structural
    invariants of what it emits, checked on the generated text (no GPU, no compiler):
    * the tile block holds 6 iterations (first / middle / last pair) of 128 MFMAs, every accumulator block a[4i : 4i+3] is the destination of
      exactly two MFMAs per iteration, and only the 64 MFMAs of the very first half start from the inline constant 0;
    * per iteration 32 fragment reads (+ 16 at the tile's entry), 16 LDS-DMA issues each preceded by its own M0 write with one other instruction
      between them, one `vmcnt(8)` + one `s_barrier` (+ the entry's `vmcnt(0)` + barrier);
    * every explicitly named VGPR / SGPR / AGPR lies inside the clobber list, M0 and SCC are declared, and a fragment register is never the
      destination of a read in the half whose MFMAs consume it."""
    text = _g4_generate(tmp_path)
    ins, pins = _g4_block(text, "G4_ASM_TILE"), _g4_block(text, "G4_ASM_PROLOGUE")
    mf = [i for i in ins if i.startswith(_G4_MF)]
    assert len(mf) == 6 * 128
    assert sum(1 for i in mf if i.endswith(", 0")) == 64 and all(i.endswith(", 0") for i in mf[:64])
    for it in range(6):
        dst = [re.match(_G4_MF + r" a\[(\d+):(\d+)\]", i).group(1) for i in mf[it * 128:(it + 1) * 128]]
        assert sorted(map(int, dst)) == sorted([4 * b for b in range(64)] * 2)
    assert sum(1 for i in ins if i.startswith("ds_read_b128")) == 16 + 6 * 32
    assert len(_g4_check_m0_spacing(ins, "global_load_lds_dwordx4")) == 6 * 16
    assert sum(1 for i in ins if i == "s_waitcnt vmcnt(8)") == 6 and sum(1 for i in ins if i == "s_waitcnt vmcnt(0)") == 1
    assert sum(1 for i in ins if i == "s_barrier") == 7
    assert sum(1 for i in pins if i.startswith("global_load_lds_dwordx4")) == 32  # K-tiles 0 and 1 of the workgroup's first tile
    _g4_check_regs(ins + pins, _g4_macros(text)["G4_CLOBBERS"])
    # ---- the paired form (split precision mode): three products per K-tile, five quarter sets
    pin = _g4_block(text, "G4P_ASM_TILE")
    pmf = [k for k, i in enumerate(pin) if i.startswith(_G4_MF)]
    assert len(pmf) == 6 * 192 and all(pin[k].endswith(", 0") for k in pmf[:64]) and sum(1 for k in pmf if pin[k].endswith(", 0")) == 64
    assert sum(1 for i in pin if i.startswith("ds_read_b128")) == 24 + 6 * 32 and sum(1 for i in pin if i.startswith("global_load_lds_dwordx4")) == 6 * 16
    assert sum(1 for i in pin if i == "s_waitcnt vmcnt(8)") == 6 and sum(1 for i in pin if i == "s_barrier") == 7
    _g4_check_regs(pin, _g4_macros(text)["G4P_CLOBBERS"])
    _g4_check_reads_spare_consumed_sets(_g4_products(pin, 64), "ds_read_b128")  # a product's reads never write a quarter set its own MFMAs consume
    _g4_check_reads_spare_consumed_sets(_g4_halves(ins), "ds_read_b128")        # a half's reads never write the fragment set its MFMAs consume


# SHA-256 of every macro body of the DEFAULT configuration (and of the accumulator read-out helpers), recorded from the generator as it stood
# before its skeleton was folded into one weaver and one loop builder.
_G4_DEFAULT_DIGESTS = {
    "G4_ASM_PROLOGUE": "0c3900fc2351b5abb73c50c952ef5906847624b835c2542911d6ecdf8bf47c78",
    "G4_ASM_TILE": "388366dab4735d6c8dcb6235b680ed67bcaeb285ece758f0fcce235fab981e98",
    "G4_CLOBBERS": "e3c2048ae4a9f916dd90a790adea04361d4807e190699bed6ebc055b30945de1",
    "G4P_ASM_PROLOGUE": "ec266d47e2a1f6d81d8319e8f147d61bb800b01028c69b3012875d1b45cf4afe",
    "G4P_ASM_TILE": "e5cef16095b057b4433e5e9c7f9714fd7a2ba881fb7df898cd5eb9d77e1173de",
    "G4P_CLOBBERS": "50639c1b4bbf8e40c059d5688bd1ca6f3a338caf8d1e77b2fd5190f8ad007ddd",
    "G4W_ASM_PROLOGUE": "1a615b233a53c819a23a016879593cd120d9095793bf8adf3316077947077332",
    "G4W_ASM_SEG": "9affd143f25fb478f5459f2a2b073214e195cc5b6e89697105943c68ab9a14cc",
    "G4W_ASM_SEG_SHORT": "8be5c51f5e09de79212be07d5f323852cb457f3d1700c3aafa56836ea0d672ee",
    "G4W_CLOBBERS": "321a3d6f9b005404f5504a74425ccfe320a6c72f3ad66912e238a9e28788eaea",
    "G4WP_ASM_PROLOGUE": "df70daee55af66cbb19bee160b5214eacf3c8a715f84f067977745682c8212c1",
    "G4WP_ASM_SEG": "45a24078015173dbf9ce4bc651763d425e587d62b6237df113db41cda2fc9929",
    "G4WP_CLOBBERS": "95b0b9a3e0f409b8001cbdf6bf71b33e7c80b9d59b2ee236f7f4a47fd3fa495b",
    "G4C6_ASM_PROLOGUE": "d8f6e17da763e6fecf014d3c3f215537e6f379200693032c4e545c2329c49f7e",
    "G4C6_ASM_TILE": "ba37dbae0603bfe70fb72952072998be2a4240f0ff63ce9f1e9997725ea29825",
    "G4C6_CLOBBERS": "a284efeba757f2dcc28eb59f988b8cc951a1daa381d7629046309e4eefea6acb",
    "G4C3_ASM_PROLOGUE": "074f311f7bb51734f42e983d39b3b5ca9a473bdd7d0f01997c6e1c3616bdef5f",
    "G4C3_ASM_TILE": "6c998deb6ce5503f606f74d7c55280f0633d3c85d547ca90be83d2f22525e37b",
    "G4C3_CLOBBERS": "e46c4fe36239dd60f912cffc95faaec6f7684cd50b78a6a40622e830d2a7c369",
    "G4CP6_ASM_PROLOGUE": "29b1eef00fb0a7e581fb48d7a72e775456ed90526e481876ad3b9fe22b615da4",
    "G4CP6_ASM_TILE": "48252b6337af9dc920b89009e2091d9d20e7ee9cf57a5ac80a9fd2d1ef2d35c6",
    "G4CP6_CLOBBERS": "745a1c99db68b6ec16f555d3b117e7f58335d4fa0d021c9f6d869ce5dd114bba",
    "G4CP3_ASM_PROLOGUE": "844a599c318b1532d1b22657399900fe0dd9374ec12b98b32e35cad862865355",
    "G4CP3_ASM_TILE": "c2bd80f2d79abb728f5337c9cfa37d7cdbdcf59cc146f20a3057457aab773d11",
    "G4CP3_CLOBBERS": "6926fdebb67ce4147779761cd33c8460e17ec62e4da8204a88c1c89e633cf216",
    "readout": "e8c0d5c79d23e481ca505130322d4d18eb172367db3e00b7e70701ba15ea60fc",
}


def test_gemm4_generator_default_output_is_pinned(tmp_path):
    """The default output of csrc/gen_gemm4.py is the schedule every measurement in profiles/ and DESIGN.md was taken with: the same macros, in
    the same order, each with the recorded body.  A wrong weave position or a register missing from a clobber list is silent corruption, so a
    change of the emitted text must be deliberate: a digest in `_G4_DEFAULT_DIGESTS` is updated ONLY together with a measurement of the new
    schedule (and the GPU tests of the engine it belongs to), never to make this test pass after an edit of the generator."""
    import hashlib

    macros = _g4_macros(_g4_generate(tmp_path))
    assert list(macros) == list(_G4_DEFAULT_DIGESTS)
    changed = [k for k, v in macros.items() if hashlib.sha256(v.encode()).hexdigest() != _G4_DEFAULT_DIGESTS[k]]
    assert not changed, changed


def test_gemm4_generator_configuration_keys(tmp_path):
    """`key=value` arguments of csrc/gen_gemm4.py (tools/gemm4_sweep.sh, tools/gemm4w_sweep.sh): an unknown key is an error that names the key
    (a typo in a sweep would otherwise measure the default schedule); every documented key changes the body of at least one macro; and the
    timing ablations hold in EVERY form: with abl_dma + abl_rd a tile / segment block keeps all its MFMAs and has no fragment read and no
    LDS-DMA issue behind its entry reads, with abl_vmw + abl_bar only the entry's barrier is left and no counted vmcnt wait."""
    r = _g4_run(tmp_path / "typo.inc", "rd_evry=2")
    assert r.returncode != 0 and "rd_evry" in r.stderr
    base_text = _g4_generate(tmp_path)
    base = _g4_macros(base_text)
    for arg in ("rd_every=2", "rd_at=1", "dm_every=7", "dm_at=4", "w_rd_at=16", "w_rd_num=1", "w_rd_den=2", "w_dm_at=2", "w_dm_every=4",
                "wp_rd_num=3", "wp_rd_den=2", "abl_rd=1", "abl_dma=1", "abl_vmw=1", "abl_bar=1"):
        m = _g4_macros(_g4_generate(tmp_path, arg))
        assert list(m) == list(base) and any(m[k] != base[k] for k in base), arg
    loops = [k for k in base if k.endswith(("_ASM_TILE", "_ASM_SEG", "_ASM_SEG_SHORT"))]
    assert len(loops) == 9
    idle = _g4_generate(tmp_path, "abl_dma=1", "abl_rd=1")
    free = _g4_generate(tmp_path, "abl_vmw=1", "abl_bar=1")
    fetch = ("ds_read_b128", "ds_read_b64_tr_b16", "buffer_load_dwordx4", "global_load_lds_dwordx4")
    for name in loops:
        ref, ins = _g4_block(base_text, name), _g4_block(idle, name)
        entry, ref_entry = [next(k for k, i in enumerate(x) if i.startswith(_G4_MF)) for x in (ins, ref)]
        assert ins[:entry] == ref[:ref_entry], name  # the entry (setup, waits, entry reads) is untouched
        assert sum(1 for i in ins if i.startswith(_G4_MF)) == sum(1 for i in ref if i.startswith(_G4_MF)), name
        assert not [i for i in ins[entry:] if i.startswith(fetch)], name
        ins = _g4_block(free, name)
        assert sum(1 for i in ins if i == "s_barrier") == 1 and [i for i in ins if i.startswith("s_waitcnt vmcnt")] == ["s_waitcnt vmcnt(0)"], name


@pytest.mark.parametrize("switch", ["IG_CONV_DIRECT", "IG_CONV8"])
@pytest.mark.parametrize("value", [None, "0", "1", "2", "abc"])
def test_engine_switches_are_read_before_any_device_call(built_lib, monkeypatch, switch, value):
    """An empty batch walks the routing of the linear and convolution entry points -- gemm8.hip, gemm8w.hip, conv_direct.hip and conv8.hip
    read their switches and decline or finish -- and returns IG_OK without a HIP call, whatever the switch holds (a non-numeric value
    counts as 0, as atoi does)."""
    lib = built_lib.load()
    if value is None:
        monkeypatch.delenv(switch, raising=False)
    else:
        monkeypatch.setenv(switch, value)
    p = ctypes.c_void_p(16)
    assert lib.ig_conv3x3_fwd(p, None, p, None, None, None, None, p, None, 0, 16, 16, 48, 48, None) == 0
    assert lib.ig_conv3x3_fwd(p, None, p, None, None, None, None, p, None, 0, 16, 16, 96, 96, None) == 0
    assert lib.ig_convT_dgrad(p, None, p, None, p, None, 0, 16, 16, 96, 48, None) == 0
    # every linear and convolution entry point, on the channel counts that pick each engine (generic, direct 48 / 96 / 96 -> 48 / 192,
    # conv8 and gemm8w's wide stages), plain and split, weight gradients with and without the bias gradient
    fused = ctypes.c_int(7)
    for entry in ("ig_linear_fwd", "ig_linear_residual_fwd", "ig_linear_dgrad", "ig_linear_dgrad_wt", "ig_linear_wgrad"):
        for N, K in ((16, 16), (768, 768), (256, 512)):
            assert getattr(lib, entry)(*_entry_args(entry, M=0, N=N, K=K)) == 0, (entry, N, K)
    for entry in ("ig_linear_dgrad", "ig_linear_dgrad_wt"):
        assert getattr(lib, entry)(*_entry_args(entry, M=0, N=768, K=768, mode=1, dact_hi=p)) == 0, entry
        assert getattr(lib, entry)(*_entry_args(entry, M=0, N=768, K=768, dx_colsum=p)) == 0, entry
    ptrs, dims = (ctypes.c_void_p * 1)(16), (ctypes.c_int * 1)(768)
    assert lib.ig_linear_wgrad_group(1, ptrs, None, ptrs, None, ptrs, dims, dims, 0, 0, None) == 0
    assert lib.ig_patch_embed_fwd(*_entry_args("ig_patch_embed_fwd", batch=0, bias=p)) == 0
    convs = [n for n in built_lib.declared_symbols() if re.match(r"ig_(conv3x3|convk|convT)_", n)]
    assert len(convs) == 11
    for entry in convs:
        header_args = re.search(r"\b%s\s*\(([^)]*)\)" % entry, open(built_lib.HEADER_PATH).read()).group(1)
        for Cin, Cout in ((16, 16), (48, 48), (96, 96), (96, 48), (192, 96), (384, 192), (256, 256)):
            for split in (False, True):
                for dbias in ((None, p) if "wgrad" in entry else (None,)):
                    over = dict(B=0, H=16, W=16, Cin=Cin, Cout=Cout, dbias=dbias, fused=ctypes.cast(ctypes.byref(fused), ctypes.c_void_p))
                    if split:
                        over.update({n: p for n in ("x_lo", "w_lo", "y_lo", "dy_lo", "dx_lo")})
                    over = {k: v for k, v in over.items() if re.search(r"\b%s\b" % k, header_args)}
                    assert getattr(lib, entry)(*_entry_args(entry, **over)) == 0, (entry, over)
                    if entry == "ig_conv3x3_fwd_stats":  # an empty batch fuses nothing
                        assert fused.value == 0, over


# ---- characterisation of the GEMM / convolution entry points' host dispatch (csrc/gemm.hip) ------------------------------------------
_PTR, _PTR8 = ctypes.c_void_p(16), ctypes.c_void_p(8)  # never dereferenced: every call below ends in a check or on an empty batch before any launch
_OPTIONAL = {"bias", "bn_scale", "bn_shift", "dbias", "dx_colsum", "dact_hi", "dact_lo", "drop_seed_dev", "stream"}
_SIZES = {"B": 1, "H": 8, "W": 8, "Cin": 16, "Cout": 16, "KS": 5, "M": 8, "N": 16, "K": 16, "D": 16, "batch": 1, "tokens_per_chip": 4,
          "ncls": 2}
_DROP = {"drop_p": 0.5, "B": 65536, "H": 256, "W": 256}  # 2^32 elements at one channel
_SPLIT = {"split": "split (lo) pointers must be given for all bf16 operands or none"}


def _entry_args(entry, **over):
    """Valid-looking arguments of ``entry`` by the parameter names in the header (optional and lo pointers NULL), then ``over``."""
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "instageo_hip.h")).read(), flags=re.S)
    params = re.search(r"\b%s\s*\(([^)]*)\)" % entry, header).group(1).split(",")
    names = [re.search(r"(\w+)\s*$", a).group(1) for a in params]
    assert set(over) <= set(names), (entry, over)
    vals = {n: (None if n in _OPTIONAL or n.endswith("_lo") else _PTR) if "*" in a else _SIZES.get(n, 0) for n, a in zip(names, params)}
    vals.update(over)
    return [vals[n] for n in names]


# (entry point, case, argument overrides, return code, ig_last_error(), *fused afterwards where the entry point has one: it is handed a
# host int holding 7): recorded by running this table against the library as it was before the entry points were folded onto shared
# helpers
_BAD_CALLS = [
    ("ig_linear_fwd", "null", {"x_hi": None}, -1, 'ig_linear_fwd: null pointer', None),
    ("ig_linear_fwd", "N-not-8", {"N": 12}, -1, 'ig_linear_fwd: N and K must be multiples of 8 (got 12, 16)', None),
    ("ig_linear_fwd", "K-not-8", {"K": 12}, -1, 'ig_linear_fwd: N and K must be multiples of 8 (got 16, 12)', None),
    ("ig_linear_fwd", "split", {"x_lo": _PTR}, -1, 'split (lo) pointers must be given for all bf16 operands or none', None),
    ("ig_linear_residual_fwd", "null", {"x_hi": None}, -1, 'ig_linear_residual_fwd: null pointer', None),
    ("ig_linear_residual_fwd", "N-not-8", {"N": 12}, -1, 'ig_linear_residual_fwd: N and K must be multiples of 8', None),
    ("ig_linear_residual_fwd", "K-not-8", {"K": 12}, -1, 'ig_linear_residual_fwd: N and K must be multiples of 8', None),
    ("ig_linear_residual_fwd", "split", {"x_lo": _PTR}, -1, 'split (lo) pointers must be given for all bf16 operands or none', None),
    ("ig_linear_dgrad", "null", {"dy_hi": None}, -1, 'ig_linear_dgrad: null pointer', None),
    ("ig_linear_dgrad", "N-not-8", {"N": 12}, -1, 'ig_linear_dgrad: N and K must be multiples of 8', None),
    ("ig_linear_dgrad", "K-not-8", {"K": 12}, -1, 'ig_linear_dgrad: N and K must be multiples of 8', None),
    ("ig_linear_dgrad", "split", {"dy_lo": _PTR}, -1, 'split (lo) pointers must be given for all bf16 operands or none', None),
    ("ig_linear_dgrad_wt", "null", {"dy_hi": None}, -1, 'ig_linear_dgrad_wt: null pointer', None),
    ("ig_linear_dgrad_wt", "N-not-8", {"N": 12}, -1, 'ig_linear_dgrad_wt: N and K must be multiples of 8', None),
    ("ig_linear_dgrad_wt", "K-not-8", {"K": 12}, -1, 'ig_linear_dgrad_wt: N and K must be multiples of 8', None),
    ("ig_linear_dgrad_wt", "split", {"dy_lo": _PTR}, -1, 'split (lo) pointers must be given for all bf16 operands or none', None),
    ("ig_linear_wgrad", "null", {"dy_hi": None}, -1, 'ig_linear_wgrad: null pointer', None),
    ("ig_linear_wgrad", "N-not-8", {"N": 12}, -1, 'ig_linear_wgrad: N and K must be multiples of 8', None),
    ("ig_linear_wgrad", "K-not-8", {"K": 12}, -1, 'ig_linear_wgrad: N and K must be multiples of 8', None),
    ("ig_linear_wgrad", "split", {"dy_lo": _PTR}, -1, 'split (lo) pointers must be given for all bf16 operands or none', None),
    ("ig_linear_fwd", "unaligned", {"x_hi": _PTR8}, -1, 'ig_linear_fwd: pointers must be 16-byte aligned', None),
    ("ig_linear_fwd", "split-in-plain-out", {"x_lo": _PTR, "w_lo": _PTR}, -1, 'ig_linear_fwd: input and output must both be split or both plain', None),
    ("ig_linear_dgrad_wt", "unaligned", {"wt_hi": _PTR8}, -1, 'ig_linear_dgrad_wt: pointers must be 16-byte aligned', None),
    ("ig_linear_dgrad_wt", "split-in-plain-out", {"dy_lo": _PTR, "wt_lo": _PTR}, -1, 'ig_linear_dgrad_wt: input and output must both be split or both plain', None),
    ("ig_linear_dgrad", "mode1-without-dact", {"mode": 1}, -1, 'ig_linear_dgrad: mode 1 needs the saved activation-derivative tensor (dact)', None),
    ("ig_linear_dgrad", "mode2", {"mode": 2, "dact_hi": _PTR}, -1, 'ig_linear_dgrad: mode 1 needs the saved activation-derivative tensor (dact)', None),
    ("ig_linear_dgrad_wt", "mode1-without-dact", {"mode": 1}, -1, 'ig_linear_dgrad_wt: mode 1 needs the saved activation-derivative tensor (dact)', None),
    ("ig_linear_dgrad_wt", "mode2", {"mode": 2, "dact_hi": _PTR}, -1, 'ig_linear_dgrad_wt: mode 1 needs the saved activation-derivative tensor (dact)', None),
    ("ig_linear_wgrad_group", "n0", {}, -1, 'ig_linear_wgrad_group: 1..16 GEMMs and non-null arrays', None),
    ("ig_linear_wgrad_group", "n17", {"n": 17}, -1, 'ig_linear_wgrad_group: 1..16 GEMMs and non-null arrays', None),
    ("ig_linear_wgrad_group", "null-array", {"n": 1, "dw": None}, -1, 'ig_linear_wgrad_group: 1..16 GEMMs and non-null arrays', None),
    ("ig_patch_embed_fwd", "null", {"pos": None}, -1, 'ig_patch_embed_fwd: null pointer', None),
    ("ig_patch_embed_fwd", "null-bias", {}, -1, 'ig_patch_embed_fwd: null pointer', None),
    ("ig_patch_embed_fwd", "D-not-8", {"bias": _PTR, "D": 12}, -1, 'ig_patch_embed_fwd: D and K must be multiples of 8', None),
    ("ig_patch_embed_fwd", "K-not-8", {"bias": _PTR, "K": 12}, -1, 'ig_patch_embed_fwd: D and K must be multiples of 8', None),
    ("ig_patch_embed_fwd", "split", {"bias": _PTR, "w_lo": _PTR}, -1, 'split (lo) pointers must be given for all bf16 operands or none', None),
    ("ig_conv3x3_fwd", "null", {"x_hi": None}, -1, 'ig_conv3x3_fwd: null pointer', None),
    ("ig_conv3x3_fwd", "Cin-not-8", {"Cin": 12}, -1, 'ig_conv3x3_fwd: channels must be multiples of 8', None),
    ("ig_conv3x3_fwd", "Cout-not-8", {"Cout": 20}, -1, 'ig_conv3x3_fwd: channels must be multiples of 8', None),
    ("ig_conv3x3_fwd", "split", {"x_lo": _PTR}, -1, 'split (lo) pointers must be given for all bf16 operands or none', None),
    ("ig_conv3x3_dgrad", "null", {"dy_hi": None}, -1, 'ig_conv3x3_dgrad: null pointer', None),
    ("ig_conv3x3_dgrad", "Cin-not-8", {"Cin": 12}, -1, 'ig_conv3x3_dgrad: channels must be multiples of 8', None),
    ("ig_conv3x3_dgrad", "Cout-not-8", {"Cout": 20}, -1, 'ig_conv3x3_dgrad: channels must be multiples of 8', None),
    ("ig_conv3x3_dgrad", "split", {"dy_lo": _PTR}, -1, 'split (lo) pointers must be given for all bf16 operands or none', None),
    ("ig_conv3x3_wgrad", "null", {"dw": None}, -1, 'ig_conv3x3_wgrad: null pointer', None),
    ("ig_conv3x3_wgrad", "Cin-not-8", {"Cin": 12}, -1, 'ig_conv3x3_wgrad: channels must be multiples of 8', None),
    ("ig_conv3x3_wgrad", "Cout-not-8", {"Cout": 20}, -1, 'ig_conv3x3_wgrad: channels must be multiples of 8', None),
    ("ig_conv3x3_wgrad", "split", {"x_lo": _PTR}, -1, 'split (lo) pointers must be given for all bf16 operands or none', None),
    ("ig_convk_fwd", "null", {"y_hi": None}, -1, 'ig_convk_fwd: null pointer', None),
    ("ig_convk_fwd", "Cin-not-8", {"Cin": 12}, -1, 'ig_convk_fwd: channels must be multiples of 8', None),
    ("ig_convk_fwd", "Cout-not-8", {"Cout": 20}, -1, 'ig_convk_fwd: channels must be multiples of 8', None),
    ("ig_convk_fwd", "split", {"w_lo": _PTR}, -1, 'split (lo) pointers must be given for all bf16 operands or none', None),
    ("ig_convk_fwd", "KS-even", {"KS": 4}, -1, 'ig_convk_fwd: kernel size 4 does not fit a 8 x 8 input', None),
    ("ig_convk_fwd", "KS-1", {"KS": 1}, -1, 'ig_convk_fwd: kernel size 1 does not fit a 8 x 8 input', None),
    ("ig_convk_fwd", "KS-11", {"KS": 11}, -1, 'ig_convk_fwd: kernel size 11 does not fit a 8 x 8 input', None),
    ("ig_convk_fwd", "KS-does-not-fit", {"KS": 7, "H": 4}, -1, 'ig_convk_fwd: kernel size 7 does not fit a 4 x 8 input', None),
    ("ig_convk_fwd", "KS-does-not-fit-W", {"KS": 9, "W": 6}, -1, 'ig_convk_fwd: kernel size 9 does not fit a 8 x 6 input', None),
    ("ig_convk_fwd", "KS-before-split", {"KS": 4, "w_lo": _PTR}, -1, 'ig_convk_fwd: kernel size 4 does not fit a 8 x 8 input', None),
    ("ig_convk_dgrad", "null", {"w_hi": None}, -1, 'ig_convk_dgrad: null pointer', None),
    ("ig_convk_dgrad", "Cin-not-8", {"Cin": 12}, -1, 'ig_convk_dgrad: channels must be multiples of 8', None),
    ("ig_convk_dgrad", "Cout-not-8", {"Cout": 20}, -1, 'ig_convk_dgrad: channels must be multiples of 8', None),
    ("ig_convk_dgrad", "split", {"dy_lo": _PTR}, -1, 'split (lo) pointers must be given for all bf16 operands or none', None),
    ("ig_convk_dgrad", "KS-even", {"KS": 4}, -1, 'ig_convk_dgrad: kernel size 4 does not fit a 8 x 8 input', None),
    ("ig_convk_dgrad", "KS-1", {"KS": 1}, -1, 'ig_convk_dgrad: kernel size 1 does not fit a 8 x 8 input', None),
    ("ig_convk_dgrad", "KS-11", {"KS": 11}, -1, 'ig_convk_dgrad: kernel size 11 does not fit a 8 x 8 input', None),
    ("ig_convk_dgrad", "KS-does-not-fit", {"KS": 7, "H": 4}, -1, 'ig_convk_dgrad: kernel size 7 does not fit a 4 x 8 input', None),
    ("ig_convk_dgrad", "KS-does-not-fit-W", {"KS": 9, "W": 6}, -1, 'ig_convk_dgrad: kernel size 9 does not fit a 8 x 6 input', None),
    ("ig_convk_dgrad", "KS-before-split", {"KS": 4, "dy_lo": _PTR}, -1, 'ig_convk_dgrad: kernel size 4 does not fit a 8 x 8 input', None),
    ("ig_convk_wgrad", "null", {"x_hi": None}, -1, 'ig_convk_wgrad: null pointer', None),
    ("ig_convk_wgrad", "Cin-not-8", {"Cin": 12}, -1, 'ig_convk_wgrad: channels must be multiples of 8', None),
    ("ig_convk_wgrad", "Cout-not-8", {"Cout": 20}, -1, 'ig_convk_wgrad: channels must be multiples of 8', None),
    ("ig_convk_wgrad", "split", {"dy_lo": _PTR}, -1, 'split (lo) pointers must be given for all bf16 operands or none', None),
    ("ig_convk_wgrad", "KS-even", {"KS": 4}, -1, 'ig_convk_wgrad: kernel size 4 does not fit a 8 x 8 input', None),
    ("ig_convk_wgrad", "KS-1", {"KS": 1}, -1, 'ig_convk_wgrad: kernel size 1 does not fit a 8 x 8 input', None),
    ("ig_convk_wgrad", "KS-11", {"KS": 11}, -1, 'ig_convk_wgrad: kernel size 11 does not fit a 8 x 8 input', None),
    ("ig_convk_wgrad", "KS-does-not-fit", {"KS": 7, "H": 4}, -1, 'ig_convk_wgrad: kernel size 7 does not fit a 4 x 8 input', None),
    ("ig_convk_wgrad", "KS-does-not-fit-W", {"KS": 9, "W": 6}, -1, 'ig_convk_wgrad: kernel size 9 does not fit a 8 x 6 input', None),
    ("ig_convk_wgrad", "KS-before-split", {"KS": 4, "dy_lo": _PTR}, -1, 'ig_convk_wgrad: kernel size 4 does not fit a 8 x 8 input', None),
    ("ig_convT_fwd", "null", {"w_hi": None}, -1, 'ig_convT_fwd: null pointer', None),
    ("ig_convT_fwd", "Cin-not-8", {"Cin": 12}, -1, 'ig_convT_fwd: channels must be multiples of 8', None),
    ("ig_convT_fwd", "Cout-not-8", {"Cout": 20}, -1, 'ig_convT_fwd: channels must be multiples of 8', None),
    ("ig_convT_fwd", "split", {"x_lo": _PTR}, -1, 'split (lo) pointers must be given for all bf16 operands or none', None),
    ("ig_convT_dgrad", "null", {"dx_hi": None}, -1, 'ig_convT_dgrad: null pointer', None),
    ("ig_convT_dgrad", "Cin-not-8", {"Cin": 12}, -1, 'ig_convT_dgrad: channels must be multiples of 8', None),
    ("ig_convT_dgrad", "Cout-not-8", {"Cout": 20}, -1, 'ig_convT_dgrad: channels must be multiples of 8', None),
    ("ig_convT_dgrad", "split", {"w_lo": _PTR}, -1, 'split (lo) pointers must be given for all bf16 operands or none', None),
    ("ig_convT_wgrad", "null", {"dy_hi": None}, -1, 'ig_convT_wgrad: null pointer', None),
    ("ig_convT_wgrad", "Cin-not-8", {"Cin": 12}, -1, 'ig_convT_wgrad: channels must be multiples of 8', None),
    ("ig_convT_wgrad", "Cout-not-8", {"Cout": 20}, -1, 'ig_convT_wgrad: channels must be multiples of 8', None),
    ("ig_convT_wgrad", "split", {"x_lo": _PTR}, -1, 'split (lo) pointers must be given for all bf16 operands or none', None),
    ("ig_conv3x3_fwd", "bn_scale-alone", {"bn_scale": _PTR}, -1, 'ig_conv3x3_fwd: bn_scale and bn_shift go together', None),
    ("ig_conv3x3_fwd", "bn_shift-alone", {"bn_shift": _PTR}, -1, 'ig_conv3x3_fwd: bn_scale and bn_shift go together', None),
    ("ig_convk_fwd", "bn_scale-alone", {"bn_scale": _PTR}, -1, 'ig_convk_fwd: bn_scale and bn_shift go together', None),
    ("ig_convk_fwd", "bn_shift-alone", {"bn_shift": _PTR}, -1, 'ig_convk_fwd: bn_scale and bn_shift go together', None),
    ("ig_convk_fwd", "split-in-plain-out", {"x_lo": _PTR, "w_lo": _PTR}, -1, 'ig_convk_fwd: input and output must both be split or both plain', None),
    ("ig_convk_fwd", "split-before-bn", {"x_lo": _PTR, "w_lo": _PTR, "bn_scale": _PTR}, -1, 'ig_convk_fwd: input and output must both be split or both plain', None),
    ("ig_conv3x3_dgrad", "dropout-2^32", {"Cin": 8, "drop_p": 0.5, "B": 65536, "H": 256, "W": 256}, -1, 'ig_conv3x3_dgrad: dropout needs < 2^32 elements', None),
    ("ig_convk_dgrad", "dropout-2^32", {"Cin": 8, "drop_p": 0.5, "B": 65536, "H": 256, "W": 256}, -1, 'ig_convk_dgrad: dropout needs < 2^32 elements', None),
    ("ig_convT_fwd", "dropout-2^32", {"Cout": 8, "drop_p": 0.5, "B": 16384, "H": 256, "W": 256}, -1, 'ig_convT_fwd: dropout needs < 2^32 elements', None),
    ("ig_conv3x3_dgrad", "split-before-dropout", {"dy_lo": _PTR, "Cin": 8, "drop_p": 0.5, "B": 65536, "H": 256, "W": 256}, -1, 'split (lo) pointers must be given for all bf16 operands or none', None),
    ("ig_conv3x3_fwd_stats", "null", {"fused": 1, "sums": None}, -1, 'ig_conv3x3_fwd_stats: null pointer', 7),
    ("ig_conv3x3_fwd_stats", "null-fused", {"fused": None}, -1, 'ig_conv3x3_fwd_stats: null pointer', None),
    ("ig_conv3x3_fwd_stats", "Cin-not-8", {"fused": 1, "Cin": 12}, -1, 'ig_conv3x3_fwd: channels must be multiples of 8', 0),
    ("ig_conv3x3_fwd_stats", "Cout-not-8", {"fused": 1, "Cout": 20}, -1, 'ig_conv3x3_fwd: channels must be multiples of 8', 0),
    ("ig_conv3x3_fwd_stats", "split-x", {"fused": 1, "x_lo": _PTR}, -1, 'split (lo) pointers must be given for all bf16 operands or none', 0),
    ("ig_conv3x3_fwd_stats", "split-w", {"fused": 1, "w_lo": _PTR, "y_lo": _PTR}, -1, 'split (lo) pointers must be given for all bf16 operands or none', 0),
    ("ig_conv3x3_cls_fwd", "null", {"fused": 1, "logits": None}, -1, 'ig_conv3x3_cls_fwd: null pointer', 7),
    ("ig_conv3x3_cls_fwd", "bn_scale-alone", {"fused": 1, "bn_scale": _PTR}, -1, 'ig_conv3x3_cls_fwd: bn_scale and bn_shift go together', 7),
    ("ig_conv3x3_cls_fwd", "split-declines", {"fused": 1, "x_lo": _PTR}, 0, '', 0),
    ("ig_conv3x3_cls_fwd", "Cin-not-Cout-declines", {"fused": 1, "Cout": 32}, 0, '', 0),
]


@pytest.mark.parametrize("entry,case,over,rc,text,fused", _BAD_CALLS, ids=[f"{c[0]}-{c[1]}" for c in _BAD_CALLS])
def test_bad_arguments_keep_their_return_code_and_text(built_lib, entry, case, over, rc, text, fused):
    lib = built_lib.load()
    flag = ctypes.c_int(7)
    if over.get("fused") == 1:
        over = dict(over, fused=ctypes.cast(ctypes.byref(flag), ctypes.c_void_p))
    assert getattr(lib, entry)(*_entry_args(entry, **over)) == rc
    if rc != 0:
        assert built_lib.last_error() == text
    assert fused is None or flag.value == fused


def test_bad_argument_table_covers_every_gemm_and_conv_entry_point(built_lib):
    want = {n for n in built_lib.declared_symbols() if re.match(r"ig_(linear_|patch_embed_fwd|conv3x3_|convk_|convT_)", n)}
    assert want == {c[0] for c in _BAD_CALLS}
