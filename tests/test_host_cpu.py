"""CPU-side checks of the product package: the C-ABI library loads and exports every symbol
the header declares, the mirror modules expose the reference's exact state_dict keys/shapes,
schedule buffers match the reference bit for bit, and nothing falls back to CPU compute."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from helpers import golden, hot_path_configs, write_stats, ROOT

import mixgan_tts_amd as mg
from mixgan_tts_amd import _lib


def _header_code():
    """include/mixgan_hip.h without its comments."""
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mixgan_hip.h")).read(), flags=re.S)


def test_header_symbols_exported():
    declared = set(re.findall(r"\b(mg_[a-z0-9_]+)\s*\(", _header_code()))
    assert declared, "no declarations parsed"
    L = ctypes.CDLL(mg.library_path())
    for name in sorted(declared):
        assert hasattr(L, name), "libmixgan_hip.so does not export " + name
    assert set(_lib.EXPORTS) == declared
    assert mg.lib().mg_version() >= 100


def test_mirrored_constants_equal_the_header():
    """Every MG_* integer of _lib has the header's value: `#define NAME value` or an enumerator `NAME = value`."""
    code = _header_code()
    header = {n: int(v) for n, v in re.findall(r"^#define[ \t]+(MG_\w+)[ \t]+\(?(-?\d+)\)?[ \t]*$", code, re.M)}
    for body in re.findall(r"\benum\s+\w+\s*\{(.*?)\}", code, re.S):
        for item in filter(None, (x.strip() for x in body.split(","))):
            m = re.fullmatch(r"(MG_\w+)\s*=\s*(-?\d+)", item)
            assert m, "enumerator without an explicit value: " + item
            header[m[1]] = int(m[2])
    mirrored = {k: v for k, v in vars(_lib).items() if k.startswith("MG_") and isinstance(v, int)}
    for family, n in (("MG_ERR_", 3), ("MG_ACT_", 5), ("MG_PACK_", 6), ("MG_DEN_L_", 9), ("MG_DEN_", 23), ("MG_FWD_", 3),
                      ("MG_PLAN_", 5), ("MG_LOSS_", 2)):
        assert len([k for k in mirrored if k.startswith(family)]) == n, family
    for k, v in sorted(mirrored.items()):
        assert k in header, k + " is not a constant of the header"
        assert v == header[k], "%s: _lib %d, header %d" % (k, v, header[k])


def _c_class(text, is_return=False):
    """Class of a C parameter declaration (`const float *w`, `long dy_bs`) or return type, as ctypes can tell them apart."""
    toks = [t for t in text.replace("*", " * ").split() if t != "const"]
    if "*" in toks:
        return "char *" if toks[:2] == ["char", "*"] else "pointer"
    kind = " ".join(toks if is_return else toks[:-1])      # a parameter's last token is its name
    return {"int": "int", "int32_t": "int", "float": "float", "long": "long", "size_t": "size_t",
            "unsigned long long": "size_t", "unsigned": "unsigned"}[kind]      # KeyError: a type this test cannot read


def _ctypes_class(ct):
    if ct is ctypes.c_char_p:
        return "char *"
    if ct is ctypes.c_void_p or issubclass(ct, ctypes._Pointer):
        return "pointer"
    return {ctypes.c_int: "int", ctypes.c_float: "float", ctypes.c_long: "long", ctypes.c_size_t: "size_t",
            ctypes.c_ulonglong: "size_t", ctypes.c_uint: "unsigned"}[ct]


def test_ctypes_signatures_match_the_header_prototypes():
    """Every prototype of the header has an entry in _lib's signature table with the same number of arguments, each of
    the same class (pointer, int, float, long, size_t / unsigned long long, unsigned), and the same return class."""
    code = re.sub(r"^[ \t]*#.*$", "", _header_code(), flags=re.M)                         # preprocessor lines
    code = re.sub(r"\b(typedef\s+struct|enum)\b[^{;]*\{.*?\}[^;]*;", "", code, flags=re.S)  # struct and enum bodies
    code = code.replace('extern "C" {', "")
    protos = {}
    for stmt in filter(None, (x.strip() for x in code.split(";"))):
        if stmt == "}":      # closes extern "C"
            continue
        m = re.fullmatch(r"(.*?)\b(mg_\w+)\s*\((.*)\)", stmt, re.S)
        assert m, "cannot read this declaration: " + stmt
        args = [] if m[3].strip() == "void" else m[3].split(",")
        protos[m[2]] = (_c_class(m[1], True), [_c_class(a) for a in args])
    sig = _lib._signatures()
    assert len(protos) >= 112 and set(protos) == set(sig)
    for name, (ret, args) in sorted(protos.items()):
        res, argtypes = sig[name]
        assert _ctypes_class(res) == ret, "%s returns %s in the header" % (name, ret)
        assert [_ctypes_class(a) for a in argtypes] == args, "%s: header %s" % (name, args)
    # and the loaded library carries exactly these
    L = mg.lib()
    for name, (res, argtypes) in sig.items():
        assert getattr(L, name).restype is res and list(getattr(L, name).argtypes) == list(argtypes), name


def test_error_strings_and_arg_checks():
    L = mg.lib()
    assert b"shape" in L.mg_error_string(_lib.MG_ERR_SHAPE)
    assert L.mg_conv_packed_floats(512, 256, 3, 1) == 16 * (256 * 3 // 8) * 256
    assert L.mg_conv_packed_floats(512, 256, 6, 0) == 0          # unsupported kernel size
    # null pointers are rejected before any launch (no GPU needed)
    assert L.mg_conv1d_fwd(None, None, None, None, None, None, 1, 8, 8, 8, 8, 1, 1, 0, 0, 1.0, 0, None) == _lib.MG_ERR_ARG
    # the entry points added for the vocoder / aux-training / grouped-gradient rows: sizes and argument checks
    assert L.mg_conv_transpose_packed_floats(512, 256, 8) == (256 * 8 // 32) * (512 * 3 // 8) * 256
    assert L.mg_conv_transpose_packed_floats(512, 256, 3) == 0                       # stride must be 2, 4 or 8
    assert L.mg_conv_transpose_pack(None, None, 512, 256, 8, None) == _lib.MG_ERR_ARG
    assert L.mg_conv_transpose1d_fwd(None, None, None, None, 1, 8, 8, 8, 2, 1.0, 1.0, None) == _lib.MG_ERR_ARG
    assert L.mg_bgemm(None, None, None, 4, 4, 4, 1, 1, 1, 4, 0, 0, 4, 1, 0, 0, 4, 0, 0, 1.0, 0, None) == _lib.MG_ERR_ARG
    assert L.mg_softmax_rows_fwd(None, None, 1, 1, 4, 1.0, None) == _lib.MG_ERR_ARG
    assert L.mg_layernorm_cm_bwd(None, None, None, None, None, 1.0, None, None, None, None, 1, 256, 4, 1e-5, None) == _lib.MG_ERR_ARG
    assert L.mg_bn_stats(None, None, None, 1, 4, 4, None) == _lib.MG_ERR_ARG
    assert L.mg_attention_fwd_f16(None, None, None, 1, 4, 2, 128, 1.0, None) == _lib.MG_ERR_ARG
    assert L.mg_diffuse_trace_bwd(None, None, None, None, None, None, None, 4, 1, 4, 80, None) == _lib.MG_ERR_ARG
    # streaming kernel (wgrad_stream.h): 256 workgroups x (tiles / 256 + 2) partial tiles of K x 128 x 128 (k=3) or
    # 128 x 256 (k=1); shapes it does not take keep the split kernel's [nsplit][G][K][Co][Ci]
    assert L.mg_conv1d_wgrad_grouped_scratch_floats(512, 256, 3, 20) == 256 * 2 * (3 * 128 * 128 + 128)   # + partial row sums
    assert L.mg_conv1d_wgrad_grouped_scratch_floats(256, 256, 1, 20) == 256 * 2 * (256 * 256 + 256)      # 1x1 wide tiles
    assert L.mg_conv1d_wgrad_grouped_scratch_floats(128, 256, 1, 20) == 256 * 2 * (128 * 256 + 128)
    assert L.mg_conv1d_wgrad_grouped_scratch_floats(512, 256, 3, 400) == 256 * (3200 // 256 + 2) * (3 * 128 * 128 + 128)
    assert L.mg_conv1d_wgrad_scratch_floats(256, 80, 1) == 128 * 256 * 80                     # 2 tiles, 256-workgroup target
    assert L.mg_conv1d_wgrad_scratch_floats(512, 128, 5) == 25 * 512 * 128 * 5                # k=5: split kernel, 20 tiles
    assert L.mg_conv1d_wgrad_grouped(None, 0, 0, None, 0, 0, None, 0, None, 2, 1, 8, 8, 8, 8, 1, 1, 0, 1.0, 0, None) == _lib.MG_ERR_ARG
    # the small diffusion, step-MLP, loss and index entry points: every one refuses null operands before it asks anything
    # of a device (name -> the integer / float arguments after the pointers, all valid)
    small = {"mg_transpose_bml": (0, 0, 1, 8, 4), "mg_transpose_bml_strided": (0, 0, 1, 8, 4, 0), "mg_diffuse_fwd": (1, 8, 4, 4),
             "mg_posterior_sample_fwd": (1, 1, 8, 4, 4), "mg_posterior_sample_bwd": (1, 1, 8, 4, 4),
             "mg_spec_affine": (1, 32, 4), "mg_act_bwd": (_lib.MG_ACT_RELU, 8), "mg_gate_bwd": (1, 2, 4), "mg_mish_fwd": (8,),
             "mg_mish_bwd": (8,), "mg_upsample_zero_act": (1, 4, 2, 8, 1.0), "mg_upsample_zero": (1, 4, 2, 8),
             "mg_step_embed": (1, 4), "mg_step_mlp_fwd": (1, 4, 6, 5), "mg_step_mlp_bwd": (1, 4, 6, 5),
             "mg_linear_small_fwd": (1, 5, 7), "mg_linear_small_bwd": (1, 5, 7), "mg_loss_sum": (0.0, 1, 8),
             "mg_loss_grad": (0.0, 1), "mg_mel_l1_fwd": (8, 4), "mg_mel_l1_bwd": (8, 4), "mg_mel_count_rows": (8, 4),
             "mg_length_regulate_fwd": (1, 4, 3, 8), "mg_length_regulate_bwd": (1, 4, 3, 8),
             "mg_word_pool_fwd": (1, 9, 4, 3, 4, 0), "mg_word_pool_bwd": (1, 9, 4, 3, 4, 0), "mg_mapping_mask": (1, 4, 8, 9),
             "mg_rel_coef": (1, 4, 8)}
    sig = _lib._signatures()
    for name, values in small.items():
        vals = iter(values)
        args = [None if a is ctypes.c_void_p else next(vals, 8) for a in sig[name][1]]
        assert getattr(L, name)(*args) == _lib.MG_ERR_ARG, name
    assert L.mg_transpose_max_m() >= 0           # 0: no device to ask


def test_bgemm_tile_choice_and_pin(monkeypatch):
    """mg_bgemm_tile: 64 x 64 workgroup tiles while the 128 x 128 ones would number fewer than 512; MG_BGEMM_TILE pins
    either form, is read on every call, and any other value is ignored."""
    L = mg.lib()
    monkeypatch.delenv("MG_BGEMM_TILE", raising=False)
    cases = [((650, 650, 8, 2), 128),        # 6 * 6 * 16 = 576 tiles: the L x L GEMMs of training from L = 641 on
             ((640, 640, 8, 2), 64),         # 5 * 5 * 16 = 400
             ((128, 1500, 8, 2), 64),        # the d-row GEMMs: 1 * 12 * 16 = 192
             ((200, 200, 16, 8), 128)]       # 2 * 2 * 128 = 512: the threshold itself
    for args, tile in cases:
        assert L.mg_bgemm_tile(*args) == tile, args
    for pin in ("64", "128"):
        monkeypatch.setenv("MG_BGEMM_TILE", pin)
        for args, _ in cases:
            assert L.mg_bgemm_tile(*args) == int(pin), (pin, args)
    for junk in ("", "0", "32", "256", "64x64", "128 ", "big"):
        monkeypatch.setenv("MG_BGEMM_TILE", junk)
        for args, tile in cases:
            assert L.mg_bgemm_tile(*args) == tile, (junk, args)


def test_le_attention_rows_thresholds():
    """mg_le_attention_rows: 16 query rows per workgroup while le_lds_bytes(16, Lk) fits the 64 KiB of dynamic LDS, else
    4, else 0.  The formula of csrc/lingenc.hip is restated here; both upper edges reach the limit exactly."""
    L = mg.lib()
    D, VCH, WMAX, LDS_MAX = 128, 32, 8, 64 * 1024

    def lds_bytes(rows, Lk):        # q rows, score rows, one V chunk, the relative-key dots
        return 4 * (rows * D + rows * Lk + D * (VCH + 1) + rows * (2 * WMAX + 1))
    assert lds_bytes(16, 615) == LDS_MAX and lds_bytes(4, 2895) == LDS_MAX
    for Lk, rows in ((615, 16), (616, 4), (2895, 4), (2896, 0), (0, 0), (-1, 0), (-2 ** 31, 0), (1, 16), (2 ** 31 - 1, 0)):
        assert L.mg_le_attention_rows(Lk) == rows, Lk
    for Lk in range(1, 3000):
        want = 16 if lds_bytes(16, Lk) <= LDS_MAX else 4 if lds_bytes(4, Lk) <= LDS_MAX else 0
        assert L.mg_le_attention_rows(Lk) == want, Lk


def test_attention_form_choice_and_pins(monkeypatch):
    """mg_attention_form: the key-split form of 128 queries while the 128-query workgroups would number fewer than 512,
    the 256-query form while its workgroups number at least 512, else the plain one; MG_ATTENTION_KSPLIT / _WIDE pin
    either choice, are read on every call, and any other value is ignored.  fp16 operands: plain or wide only."""
    L = mg.lib()
    PLAIN, KS64, KS128, WIDE = _lib.MG_ATTN_PLAIN128, _lib.MG_ATTN_KSPLIT64, _lib.MG_ATTN_KSPLIT128, _lib.MG_ATTN_WIDE256
    assert (PLAIN, KS64, KS128, WIDE) == (0, 1, 2, 3)
    for v in ("MG_ATTENTION_KSPLIT", "MG_ATTENTION_WIDE"):
        monkeypatch.delenv(v, raising=False)
    # (B, L, n_head) -> (fp32 form, fp16 form)
    cases = [((16, 1000, 2), KS128, PLAIN),      # 8 * 32 = 256 workgroups of 128 queries
             ((16, 4000, 2), WIDE, WIDE),        # 16 * 32 = 512 workgroups of 256 queries: the threshold itself
             ((16, 3840, 2), PLAIN, PLAIN),      # 480 wide workgroups, 960 plain ones
             ((16, 3841, 2), WIDE, WIDE),        # 16 wide tiles again
             ((16, 2048, 2), PLAIN, PLAIN),      # exactly 512 plain workgroups
             ((16, 2047, 2), PLAIN, PLAIN),      # the same count
             ((16, 1921, 2), PLAIN, PLAIN),
             ((16, 1920, 2), KS128, PLAIN),      # 15 * 32 = 480
             ((2, 1, 3), KS128, PLAIN), ((2, 700, 3), KS128, PLAIN)]
    for args, f32, f16 in cases:
        assert L.mg_attention_form(*args, 0) == f32, args
        assert L.mg_attention_form(*args, 1) == f16, args
    # every pin, at every size
    for ks, wide, f32 in (("0", "0", PLAIN), ("0", "1", WIDE), ("1", "0", KS64), ("1", "1", KS64), ("2", "0", KS128),
                          ("2", "1", KS128)):
        monkeypatch.setenv("MG_ATTENTION_KSPLIT", ks)
        monkeypatch.setenv("MG_ATTENTION_WIDE", wide)
        for args, _, _ in cases:
            assert L.mg_attention_form(*args, 0) == f32, (ks, wide, args)
            assert L.mg_attention_form(*args, 1) == (WIDE if wide == "1" else PLAIN), (ks, wide, args)
    # one pin alone: the other choice stays with the rule
    monkeypatch.delenv("MG_ATTENTION_WIDE")
    monkeypatch.setenv("MG_ATTENTION_KSPLIT", "0")
    for args, f32, f16 in cases:
        assert L.mg_attention_form(*args, 0) == f16, args       # without the key split fp32 follows the fp16 rule
        assert L.mg_attention_form(*args, 1) == f16, args
    monkeypatch.delenv("MG_ATTENTION_KSPLIT")
    monkeypatch.setenv("MG_ATTENTION_WIDE", "1")
    for args, f32, _ in cases:
        assert L.mg_attention_form(*args, 0) == (f32 if f32 == KS128 else WIDE), args
        assert L.mg_attention_form(*args, 1) == WIDE, args
    # anything else is ignored
    for junk in ("", "3", "9", "-1", "01", "2 ", "1x", "yes"):
        monkeypatch.setenv("MG_ATTENTION_KSPLIT", junk)
        monkeypatch.setenv("MG_ATTENTION_WIDE", junk if junk != "01" else "10")
        for args, f32, f16 in cases:
            assert L.mg_attention_form(*args, 0) == f32, (junk, args)
            assert L.mg_attention_form(*args, 1) == f16, (junk, args)
    for bad in ((0, 4, 2), (2, 0, 2), (2, 4, 0), (-1, 4, 2)):
        assert L.mg_attention_form(*bad, 0) == _lib.MG_ERR_SHAPE and L.mg_attention_form(*bad, 1) == _lib.MG_ERR_SHAPE


def test_schedule_matches_reference_bits():
    g = golden("schedule")
    for mode, T in [("vpsde", 1), ("vpsde", 4), ("vpsde", 100), ("vpsde", 1000), ("linear", 4), ("cosine", 4)]:
        b = mg.diffusion_buffers(mg.beta_schedule(mode, T, 0.1, 40, 0.008))
        for k, v in b.items():
            np.testing.assert_array_equal(v, g["%s_%d/%s" % (mode, T, k)])


@pytest.mark.parametrize("ms", [False, True])
def test_state_dict_keys_match_reference(manifest, tmp_path, ms):
    e = golden("elementwise")
    stats = write_stats(tmp_path, e["spec_min"], e["spec_max"])
    gd = mg.GaussianDiffusion(*hot_path_configs("naive", 4, multi_speaker=ms, stats_dir=stats))
    ref = manifest["diffusion_naive_ms%d" % int(ms)]["state_dict"]
    mine = {k: list(v.shape) for k, v in gd.state_dict().items()}
    assert mine == ref
    # parameter registration order (optimizer state indices) follows the reference too
    man = manifest["diffusion_naive_ms%d" % int(ms)]
    assert [k for k, _ in gd.named_parameters()] == man["param_order"]
    assert list(gd.state_dict().keys()) == man["state_dict_order"]
    g = golden("schedule")
    for k in mg.schedule.BUFFER_NAMES:
        np.testing.assert_array_equal(getattr(gd, k).numpy(), g["vpsde_4/" + k])
    # zero-initialised output projection (model/modules.py:418)
    assert float(gd.denoise_fn.output_projection.conv.weight.abs().sum()) == 0.0


def test_no_cpu_fallback(tmp_path):
    e = golden("elementwise")
    stats = write_stats(tmp_path, e["spec_min"], e["spec_max"])
    gd = mg.GaussianDiffusion(*hot_path_configs("naive", 4, stats_dir=stats))
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(mg.MixganHipError):
        gd.denoise_fn(torch.zeros(1, 1, 80, 16), torch.zeros(1, dtype=torch.long), torch.zeros(1, 256, 16), None)
    with pytest.raises(mg.MixganHipError):
        gd(None, torch.zeros(1, 16, 256), None, torch.zeros(1, 16, dtype=torch.bool))


def test_product_does_not_import_oracle():
    pkg = os.path.join(ROOT, "mixgan-tts_amd")
    for dirpath, _, files in os.walk(pkg):
        for fn in files:
            if fn.endswith((".py", ".hip", ".h", ".cpp")):
                txt = open(os.path.join(dirpath, fn)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", txt, re.M), fn


def test_oracle_is_only_used_as_a_checker():
    """Outside tests/ the oracle may be imported only by __graft_entry__.smoke() and bench.py's cpu_baseline leg
    (task statement, section 3); tools/ and the package must not touch it, and nothing at the repo root reads
    /root/reference at run time (it does not exist on the GPU box)."""
    allowed = {"bench.py": "def cpu_baseline", "__graft_entry__.py": "def smoke"}
    pat = re.compile(r"^\s*(from|import)\s+oracle\b", re.M)
    for dirpath, dirs, files in os.walk(ROOT):
        dirs[:] = [d for d in dirs if d not in (".git", "tests", "oracle", "gpurun_out", "__pycache__", ".pytest_cache")]
        for fn in files:
            if not fn.endswith(".py"):
                continue
            path = os.path.join(dirpath, fn)
            txt = open(path).read()
            rel = os.path.relpath(path, ROOT)
            for m in pat.finditer(txt):
                assert rel in allowed, "%s imports the oracle" % rel
                # the import must sit inside the one function that is allowed to use it
                head = txt[:m.start()]
                last_def = head.rfind("\ndef ")
                assert txt[last_def + 1:].startswith(allowed[rel]), "%s: oracle import outside %s" % (rel, allowed[rel])
    for fn in ("bench.py", "__graft_entry__.py"):
        assert "/root/reference" not in open(os.path.join(ROOT, fn)).read(), fn
    for dirpath, _, files in os.walk(os.path.join(ROOT, "mixgan-tts_amd")):
        for fn in files:
            if fn.endswith(".py"):
                assert "/root/reference" not in open(os.path.join(dirpath, fn)).read(), fn


def test_get_model_and_checkpoint_round_trip(tmp_path):
    """utils/model.py:12-53 + train.py:252-267: the 8-tuple of the training entry, the checkpoint keys, a strict
    restore of G / D / optimizer / scheduler state, eval-mode return, and the aux -> shallow optimizer restart.
    Construction and state handling only -- no kernel is launched, so it runs without a GPU."""
    import types
    e = golden("elementwise")
    stats = write_stats(tmp_path, e["spec_min"], e["spec_max"])
    args, pre, mc, tr = hot_path_configs("shallow", 4, stats_dir=stats)
    tr = dict(tr)
    tr["path"] = {"ckpt_path": str(tmp_path / "ckpt")}
    tr["step"] = {"total_step_aux": 7}
    tr["optimizer_fs2"] = {"betas": [0.9, 0.98], "eps": 1e-9, "weight_decay": 0.0, "warm_up_step": 4000,
                           "anneal_steps": [300000], "anneal_rate": 0.3}
    configs = (pre, mc, tr)
    a0 = types.SimpleNamespace(model="shallow", restore_step=0)
    model, D, optG_fs2, optG, optD, sdlG, sdlD, epoch = mg.get_model(a0, configs, "cpu", train=True)
    assert epoch == 1 and model.training and D.training and isinstance(optG_fs2, mg.ScheduledOptim)
    assert mg.get_param_num(model) == sum(p.numel() for p in model.parameters()) > 20_000_000
    # give the optimizers some state, then save as train.py does
    for p in list(model.parameters())[:3] + list(D.parameters())[:3]:
        p.grad = torch.ones_like(p)
    optG.step(); optD.step(); optG_fs2.step(); sdlG.step(); sdlD.step()
    path = mg.save_checkpoint(tr, 3, 5, model, D, optG_fs2, optG, optD, sdlG, sdlD)
    ck = torch.load(path, weights_only=True)
    assert tuple(ck.keys()) == ("epoch", "G", "D", "optG_fs2", "optG", "optD", "sdlG", "sdlD")
    a3 = types.SimpleNamespace(model="shallow", restore_step=3)
    m2, D2, f2, g2, d2, sg2, sd2, ep2 = mg.get_model(a3, configs, "cpu", train=True)
    assert ep2 == 5
    for k, v in model.state_dict().items():
        assert torch.equal(v, m2.state_dict()[k]), k
    for k, v in D.state_dict().items():
        assert torch.equal(v, D2.state_dict()[k]), k
    assert g2.state_dict()["state"].keys() == optG.state_dict()["state"].keys() and len(g2.state_dict()["state"]) == 3
    assert sg2.state_dict()["last_epoch"] == 1 and f2.current_step == 3
    assert f2._optimizer.state_dict()["state"].keys() == optG_fs2._optimizer.state_dict()["state"].keys()
    # eval entry (synthesize.py:245)
    m3 = mg.get_model(a3, configs, "cpu", train=False)
    assert not m3.training and torch.equal(m3.state_dict()["mel_linear.weight"], model.state_dict()["mel_linear.weight"])
    # restore_step == total_step_aux: weights restored, optimizers start fresh (utils/model.py:41)
    mg.save_checkpoint(tr, 7, 9, model, D, optG_fs2, optG, optD, sdlG, sdlD)
    a7 = types.SimpleNamespace(model="shallow", restore_step=7)
    _, _, f7, g7, *_ = mg.get_model(a7, configs, "cpu", train=True)
    assert len(g7.state_dict()["state"]) == 0 and f7.current_step == 7


def test_in_kernel_noise_key_differs_per_rank_and_workspaces_are_numbered(monkeypatch):
    """Ranks that seed torch identically must not draw identical in-kernel noise (the Philox key mixes rank and device
    in), and every workspace instance gets its own stream number (the high word of the Philox offset)."""
    from mixgan_tts_amd import denoiser as D
    dev0, dev1 = torch.device("cuda", 0), torch.device("cuda", 1)
    salts = set()
    for rank in range(8):
        monkeypatch.setenv("RANK", str(rank))
        salts.add(D._rank_salt(dev0))
        salts.add(D._rank_salt(dev1))
    assert len(salts) == 16 and all(0 <= s < 2 ** 64 for s in salts)
    a, b = next(D._NOISE_STREAMS), next(D._NOISE_STREAMS)
    assert b == a + 1 and a >= 1
