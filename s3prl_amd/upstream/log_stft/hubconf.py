"""hub entry of the STFT-magnitude upstream under the reference's name and signature (s3prl/upstream/log_stft/hubconf.py):
``stft_mag(model_config, *args, **kwargs)``.  ``model_config`` is a yaml file in the reference's schema or the parsed dict;
``STFT_MAG`` / ``LOG_STFT_MAG`` state the settings of the reference's two files."""

import os

from .expert import UpstreamExpert as _UpstreamExpert

STFT_MAG = {"feat_type": "spectrogram",
            "spectrogram": {"n_fft": 512, "hop_length": 320, "win_length": 512, "window": "hann", "center": True, "log": False}}
LOG_STFT_MAG = {"feat_type": "spectrogram", "spectrogram": dict(STFT_MAG["spectrogram"], log=True)}


def stft_mag(model_config, *args, **kwargs):
    assert isinstance(model_config, dict) or os.path.isfile(model_config)
    return _UpstreamExpert(model_config, *args, **kwargs)
