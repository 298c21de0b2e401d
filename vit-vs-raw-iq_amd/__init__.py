"""vit-vs-raw-iq_amd: MI355X-native (gfx950) training path for the ViT and raw-IQ modulation
classifiers of aliftffd/ViT-vs-Raw-IQ.

Import name: `vit_vs_raw_iq_amd` (the directory name contains hyphens; the repo-root module
`vit_vs_raw_iq_amd.py` registers this package under that name).

  modules   -- the reference's nn.Module surface (AMCTransformer x2, Encoder x2, layer shells)
  trainer   -- fused native training step (CE + backward + clip + AdamW) and data-parallel driver
  data      -- seeded synthetic IQ frames (the reference ships no data)
  attention_maps -- per-layer attention probabilities and attention rollout from the fused forward pass
  saliency  -- input gradients of the fused model: gradient saliency, integrated gradients
  relevance -- class-specific attention relevance (gradient-weighted rollout) and gradient-weighted attention maps
  adversarial -- FGSM / PGD attacks on the model input and accuracy-versus-epsilon curves
  impairments -- channel impairments on the device (phase, frequency offset, shift, gain, AWGN): augmentation and accuracy curves
  synth     -- labelled synthetic frames made on the device as a keyed stream (FrameSynth, SynthStream, train_on_stream)
  waveform  -- pulse-shaped frames on the device: RRC shaping, true OQPSK, GMSK as CPM, timing phase, multipath (ShapedSynth)
  fading    -- fading channel on the device: Doppler-spread taps (Clarke's model) and a sample-clock offset behind any raw frames
               (Fading, FadedSynth, fading_curve)
  frontend  -- what the three image front ends below share (FrontEnd: checks, one autograd function, launch, fit, table cache)
               and front_end, the `spectrogram=` argument of the input paths
  spectrogram -- spectrogram front end on the device: (B, 2, len) frames -> the (B, 1, n_fft, width) image of the ViT, differentiable
  cyclic    -- cyclic-spectrum front end on the device: (B, 2, len) frames -> the (B, C, n_fft, n_fft) spectral correlation image,
               differentiable on request
  constellation -- constellation front end on the device: (B, 2, len) points -> the (B, 1, height, width) density image, differentiable
  receiver  -- receiver on the device: matched filter, timing estimate, one sample per symbol, differentiable (Receiver, ReceivedSynth)
  carrier   -- carrier recovery on the device: blind frequency and phase estimate from the M-th-power line, derotation,
               differentiable (Carrier), and Synchronised, a front end behind it
  equaliser -- blind equaliser on the device: block constant-modulus descent of an L-tap filter per frame, differentiable
               (Equaliser); goes in front of the carrier recovery (Synchronised(equaliser=), ReceivedSynth(equaliser=, carrier=))
  equaliser_track -- tracking equaliser on the device: the same descent per overlapping segment of the frame, from the block
               solution, and a filter whose weights are interpolated over time (TrackingEqualiser, a subclass of Equaliser: goes
               wherever that one goes); for channels that move within a frame (fading)
  likelihood -- likelihood classifier on the device: the classical AMC baseline over the candidate constellations and a table of
               carrier rotations (LikelihoodClassifier, noise_for); evaluation.evaluate_likelihood_with_confusion writes its report
  likelihood_em -- hybrid likelihood classifier on the device: the likelihood test with gain, phase and noise unknown, EM per frame
               and class from a table of starts, and a blind SNR estimate (HybridLikelihoodClassifier);
               evaluation.evaluate_hybrid_with_confusion writes its report
  cumulants -- cumulant classifier on the device: the feature-based AMC baseline, ten rotation-invariant features of the cumulants
               up to order eight against a centroid per class, blind or with a known noise variance, fitted from generated frames
               (CumulantClassifier), and the true gradient of its scores and features with respect to the symbols;
               evaluation.evaluate_cumulants_with_confusion writes its report
  _native   -- ctypes binding of include/iqvit.h  (libiqvit.so; no fallback)
  ViT.models.amc_transformer / transformer_rawIQ.models.transformer_rawIQ
            -- import paths used by the reference's scripts (hyperparameter_tuning.py:19,37)
"""
from .modules import (AMCTransformerViT, AMCTransformerRawIQ, EncoderViT, EncoderRawIQ, EncoderLayer, LayerNorm,
                      MultiHeadAttention, PositionwiseFeedForward, ScaleDotProductAttention, PatchEmbedding,
                      SequenceEmbedding, NativePlan)
from ._native import IqError, LIB_PATH
from .attention_maps import attention_maps, attention_rollout, rollout_to_input
from .saliency import input_gradient, integrated_gradients
from .relevance import attention_relevance, grad_attention_maps
from .adversarial import fgsm, pgd, robustness_curve, transfer_table
from .impairments import Impairments, impair, impair_reference, impairment_curve
from .synth import FrameSynth, SynthStream, synth_reference, train_on_stream
from .waveform import ShapedSynth, gmsk_table, rrc_table, waveform_reference
from .fading import FadedSynth, Fading, fading_curve, fading_reference, interp_table
from .spectrogram import Spectrogram, spectrogram_reference, spectrogram_reference_bwd
from .cyclic import CyclicSpectrum, cyclic_reference, cyclic_reference_bwd
from .constellation import Constellation, constellation_reference, constellation_reference_bwd
from .receiver import (Receiver, ReceivedSynth, mf_table, receiver_reference, receiver_reference_bwd,
                       transmitted_index)
from .carrier import Carrier, Synchronised, carrier_reference, carrier_reference_bwd, dft_tables
from .equaliser import Equaliser, equaliser_reference, equaliser_reference_bwd
from .equaliser_track import (TrackingEqualiser, equaliser_track_reference, equaliser_track_reference_bwd, segment_step_reference,
                              taper_table)
from .likelihood import LikelihoodClassifier, likelihood_reference, noise_for
from .likelihood_em import HybridLikelihoodClassifier, likelihood_em_reference
from .cumulants import FEATURE_NAMES, CumulantClassifier, cumulant_features_of, cumulants_reference, cumulants_reference_bwd

__all__ = ["AMCTransformerViT", "AMCTransformerRawIQ", "EncoderViT", "EncoderRawIQ", "EncoderLayer", "LayerNorm",
           "MultiHeadAttention", "PositionwiseFeedForward", "ScaleDotProductAttention", "PatchEmbedding",
           "SequenceEmbedding", "NativePlan", "IqError", "LIB_PATH", "attention_maps", "attention_rollout",
           "rollout_to_input", "input_gradient", "integrated_gradients", "attention_relevance", "grad_attention_maps", "fgsm",
           "pgd", "robustness_curve", "transfer_table", "Impairments", "impair", "impair_reference", "impairment_curve", "FrameSynth",
           "SynthStream", "synth_reference", "train_on_stream", "Spectrogram", "spectrogram_reference", "spectrogram_reference_bwd",
           "ShapedSynth", "rrc_table", "gmsk_table", "waveform_reference", "Receiver", "ReceivedSynth", "mf_table", "receiver_reference",
           "receiver_reference_bwd", "transmitted_index", "CyclicSpectrum", "cyclic_reference", "cyclic_reference_bwd",
           "Constellation", "constellation_reference", "constellation_reference_bwd", "Carrier", "Synchronised", "carrier_reference",
           "carrier_reference_bwd", "dft_tables", "Equaliser", "equaliser_reference", "equaliser_reference_bwd",
           "LikelihoodClassifier", "likelihood_reference", "noise_for", "HybridLikelihoodClassifier",
           "likelihood_em_reference", "CumulantClassifier", "cumulants_reference", "cumulants_reference_bwd",
           "cumulant_features_of", "FEATURE_NAMES", "Fading", "FadedSynth", "fading_curve", "fading_reference", "interp_table",
           "TrackingEqualiser", "equaliser_track_reference", "equaliser_track_reference_bwd", "segment_step_reference", "taper_table"]
