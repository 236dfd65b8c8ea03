"""mixgan-tts_amd -- MI355X-native (gfx950) diffusion hot path of MixGAN-TTS.

Host-side mirror of the reference's module surface (same class names, constructor and
forward signatures, state_dict keys) over hand-written HIP kernels reached through the C ABI
in include/mixgan_hip.h.  Import as `mixgan_tts_amd` (see ../mixgan_tts_amd.py).

There is no CPU or eager-PyTorch fallback: a forward on a machine without the built
`libmixgan_hip.so` / without a GPU raises.
"""
from ._lib import lib, library_path, MixganHipError  # noqa: F401
from .schedule import beta_schedule, diffusion_buffers  # noqa: F401
from .blocks import ConvNorm, LinearNorm, DiffusionEmbedding, Mish, ResidualBlock  # noqa: F401
from .denoiser import Denoiser  # noqa: F401
from .diffusion import GaussianDiffusion  # noqa: F401
from .discriminator import JCUDiscriminator  # noqa: F401
from . import ops, autograd, losses, distributed  # noqa: F401
from .train_step import HotPathTrainer, AuxTrainer  # noqa: F401
from . import lingops, vocoder, data, audio  # noqa: F401
from . import optimizer  # noqa: F401
from .optimizer import ScheduledOptim, FlatAdam  # noqa: F401
from .distributed import GradBucket, BatchShape, ShardCounts, exchange_batch_shape  # noqa: F401
from .mixgantts import MixGANTTS, get_mask_from_lengths  # noqa: F401
from .transformer import Decoder, FFTBlock, PostNet, MultiHeadAttention, PositionwiseFeedForward  # noqa: F401
from .model_io import get_model, save_checkpoint, get_param_num  # noqa: F401
from .linguistic_encoder import LinguisticEncoder  # noqa: F401
from .losses import LinguisticEncoderLoss  # noqa: F401
from .melgan import MelGANGenerator, MelVocoder  # noqa: F401
from . import speaker_embedder  # noqa: F401
from .speaker_embedder import (DeepSpeakerModel, PreDefinedEmbedder, DeepSpeakerCheckpointRequired,  # noqa: F401
                               save_speaker_embeddings)

from . import corpusops, preprocessor  # noqa: F401
from .corpusops import attn_prior, phoneme_average  # noqa: F401
from .preprocessor import Preprocessor, PitchExtractorRequired, read_textgrid, write_textgrid  # noqa: F401
from . import prepare_align  # noqa: F401
from .audio import resample, resample_filter, peak_normalize_int16  # noqa: F401
from . import pitch  # noqa: F401
from .pitch import yin_candidates, pitch_track, extract_f0, native_pitch, PitchGeometryError  # noqa: F401
from . import aligner  # noqa: F401
from .aligner import (ForcedAligner, AlignGeometryError, emissions, viterbi_align, gaussian_stats,  # noqa: F401
                      read_lexicon)
from . import metrics  # noqa: F401
from .metrics import (DtwGeometryError, mel_cepstra, dtw, mel_cepstral_distortion, f0_metrics,  # noqa: F401
                      synthesis_report, evaluate_model)
from . import vocoder_train  # noqa: F401
from .vocoder_train import GeneratorTrainer, VocoderGANTrainer, sample_segments  # noqa: F401
from .losses import hifigan_discriminator_loss, hifigan_generator_loss, hifigan_feature_loss  # noqa: F401
from . import hifigan_discriminators  # noqa: F401
from .hifigan_discriminators import DiscriminatorS, MultiScaleDiscriminator  # noqa: F401
from .hifigan_discriminators import DiscriminatorP, MultiPeriodDiscriminator  # noqa: F401
from . import melgan_discriminators  # noqa: F401
from .losses import melgan_discriminator_loss, melgan_generator_loss, melgan_feature_loss  # noqa: F401

__version__ = "0.1.0"
