"""hub entries of the baseline upstream in the reference's naming (s3prl/upstream/baseline/hubconf.py:19-85).  The
hyper-parameters of the reference's ``fbank.yaml`` / ``fbank_no_cmvn.yaml`` (80 mel bins, 25 ms window, 10 ms shift, log; delta
order 2 over 5 frames; CMVN on / off), ``spectrogram.yaml``, ``mfcc.yaml``, ``mel.yaml`` and ``linear.yaml`` are stated here as
dicts; ``baseline_local`` still takes a yaml file in the same schema."""

import os

from .expert import UpstreamExpert as _UpstreamExpert


def _fbank_config(use_cmvn: bool) -> dict:
    return {
        "kaldi": {"feat_type": "fbank",
                  "fbank": {"num_mel_bins": 80, "frame_length": 25.0, "frame_shift": 10.0, "use_log_fbank": True}},
        "delta": {"order": 2, "win_length": 5},
        "cmvn": {"use_cmvn": use_cmvn},
    }


def _kaldi_config(feat_type: str, options: dict, order: int) -> dict:
    return {"kaldi": {"feat_type": feat_type, feat_type: dict(options, frame_length=25.0, frame_shift=10.0)},
            "delta": {"order": order, "win_length": 5}, "cmvn": {"use_cmvn": True}}


def _preprocessor_config(feat_type: str) -> dict:
    return {"win_ms": 25, "hop_ms": 10, "n_freq": 201, "n_mels": 80, "n_mfcc": 13,
            "input": {"feat_type": feat_type, "channel": 0, "log": True, "delta": 0, "cmvn": True}}


def baseline_local(model_config, *args, **kwargs):
    assert isinstance(model_config, dict) or os.path.isfile(model_config)
    return _UpstreamExpert(model_config, *args, **kwargs)


def baseline(*args, **kwargs):
    return fbank(*args, **kwargs)


def fbank(*args, **kwargs):
    kwargs["model_config"] = _fbank_config(True)
    return baseline_local(*args, **kwargs)


def fbank_no_cmvn(*args, **kwargs):
    kwargs["model_config"] = _fbank_config(False)
    return baseline_local(*args, **kwargs)


def spectrogram(*args, **kwargs):
    kwargs["model_config"] = _kaldi_config("spectrogram", {}, 0)
    return baseline_local(*args, **kwargs)


def mfcc(*args, **kwargs):
    kwargs["model_config"] = _kaldi_config("mfcc", {"num_ceps": 13}, 2)
    return baseline_local(*args, **kwargs)


def mel(*args, **kwargs):
    kwargs["model_config"] = _preprocessor_config("mel")
    return baseline_local(*args, **kwargs)


def linear(*args, **kwargs):
    kwargs["model_config"] = _preprocessor_config("linear")
    return baseline_local(*args, **kwargs)
