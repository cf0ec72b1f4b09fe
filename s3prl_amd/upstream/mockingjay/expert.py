"""MI355X-native stand-in for ``s3prl/upstream/mockingjay/expert.py::UpstreamExpert`` (Mockingjay, TERA and AudioALBERT share it: same
constructor / forward / get_downsample_rates contract; the forward runs in libs3enc's HIP kernels, csrc/logmel.hip, csrc/fbank.hip
and csrc/mockingjay.hip).

``forward(wavs)`` returns ``hidden_states`` = the input representation followed by every layer's output (``num_hidden_layers + 1``
states of ``(B, T, hidden)``) and ``last_hidden_state``, plus ``hidden_state_{i}`` and ``_hidden_states_info``.  Rows at or behind an
utterance's own frame count are padding: finite and deterministic, not the reference's values.

``options_config`` (the reference's yaml of string flags) is accepted.  The HIP path is an inference-only forward with dropout
off, so the options that change the forward are refused by name: ``permute_input``, ``no_grad: False`` fine-tuning together with
``.train()`` (the shared guard of ``HipUpstreamExpert``), ``spec_aug`` in training, a ``dropout`` override and
``output_hidden_states: False``."""

import yaml

from ..base import HipUpstreamExpert


def _flag(value) -> bool:
    return str(value).strip().lower() in ("y", "yes", "t", "true", "on", "1")


class UpstreamExpert(HipUpstreamExpert):
    family = "mockingjay"

    def __init__(self, ckpt: str = None, options_config: str = None, **kwargs):
        options = {"load_pretrain": "True", "no_grad": "False", "dropout": "default", "spec_aug": "False", "spec_aug_prev": "True",
                   "output_hidden_states": "True", "permute_input": "False"}  # mockingjay/expert.py:38-46
        if options_config is not None:
            with open(options_config, "r") as f:
                options = yaml.load(f, Loader=yaml.FullLoader)
        if _flag(options.get("permute_input", "False")):
            raise NotImplementedError("options: permute_input=True ((T, B, D) tensors) is not built: the expert is handed waveforms")
        if not _flag(options.get("load_pretrain", "True")):
            raise NotImplementedError("options: load_pretrain=False (a randomly initialised model) is not built")
        if not _flag(options.get("output_hidden_states", "True")):
            raise NotImplementedError("options: output_hidden_states=False is not built (the expert returns every state)")
        if str(options.get("dropout", "default")) != "default":
            raise NotImplementedError("options: a dropout override is a fine-tuning option; the HIP forward is inference-only")
        self.spec_aug = _flag(options.get("spec_aug", "False"))
        self.no_grad = _flag(options.get("no_grad", "False"))
        if not self.no_grad and not _flag(options.get("spec_aug_prev", "True")):
            raise RuntimeError("Only one of them can be set False!")  # builder.py:86-87
        super().__init__(ckpt, **kwargs)

    def get_downsample_rates(self, key: str = None) -> int:
        return 160  # mockingjay/expert.py:57-58

    def _states_info(self, n: int):
        return tuple(f"hidden_states[{i}]" for i in range(n))

    def forward(self, wavs):
        if self.training and self.spec_aug:
            raise NotImplementedError("options: spec_aug=True in training mode changes the forward and is not built")
        return super().forward(wavs)
