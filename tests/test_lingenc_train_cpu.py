"""Training the native LinguisticEncoder, without a GPU: LinguisticEncoderLoss (losses.py) on the encoder outputs the
REAL reference recorded in train mode (tests/golden/make_golden_lingenc_train.py) reproduces the reference's own
duration / pitch / energy / helper terms for dga and ctc, and the train-mode forward's argument errors."""
import pytest
import torch

from helpers import golden
from lingenc_helpers import configs, encoder_inputs
from lingenc_train_helpers import TRAIN_CASES, train_manifest, fixture_loss_inputs, loss_terms_close


@pytest.mark.parametrize("name", TRAIN_CASES)
def test_loss_terms_match_reference_fixture(tmp_path, name):
    import mixgan_tts_amd as mg
    g = golden(name)
    pre, mc, tr = configs(train_manifest(), name, tmp_path)
    loss = mg.LinguisticEncoderLoss(pre, mc, tr)
    slots, batch = fixture_loss_inputs(g, "cpu")
    total = loss(batch, slots, 1)
    loss_terms_close(loss.last, g, 1e-5)
    assert float(total) == pytest.approx(float(g["loss/total"]), rel=1e-5)


def test_loss_is_zero_for_shallow_and_switches_ctc_weight(tmp_path):
    import mixgan_tts_amd as mg
    name = "lingenc_train_ctc"
    g = golden(name)
    pre, mc, tr = configs(train_manifest(), name, tmp_path)
    slots, batch = fixture_loss_inputs(g, "cpu")
    assert float(mg.LinguisticEncoderLoss(pre, mc, tr, model="shallow")(batch, slots, 1)) == 0.0
    tr["aligner"]["ctc_weight_end"] = 0.0
    loss = mg.LinguisticEncoderLoss(pre, mc, tr)
    after = loss.terms(batch, slots, tr["step"]["ctc_step"] + 1)
    assert float(after["helper_loss"]) == 0.0 and float(after["ctc_loss"]) > 0


def test_training_forward_argument_errors(tmp_path):
    """Training runs on the HIP path only (CPU tensors raise an error that is both the library's and
    NotImplementedError, and points at the reference's encoder for CPU training), and a sequence longer than
    max_seq_len raises ValueError before anything runs."""
    import mixgan_tts_amd as mg
    name = "lingenc_train_dga"
    pre, mc, tr = configs(train_manifest(), name, tmp_path)
    enc = mg.LinguisticEncoder(pre, mc, tr).train()
    args = list(encoder_inputs(golden(name), "cpu"))
    with pytest.raises(mg._lib.MixganHipError, match="no CPU fallback") as e:
        enc(*args)
    assert isinstance(e.value, NotImplementedError) and "inject the reference" in str(e.value)
    enc.max_seq_len = args[0].shape[1] - 1
    with pytest.raises(ValueError, match="max_seq_len"):
        enc(*args)
    enc.eval()
    with torch.no_grad():
        with pytest.raises(mg._lib.MixganHipError):
            enc(*args)
