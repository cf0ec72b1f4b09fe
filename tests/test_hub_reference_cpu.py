"""The registration promise of INTEGRATION.md §1 against the reference's ``s3prl.hub`` / hubconf surface, as recorded in
``tests/golden/reference_hub.json`` (``make_golden.py reference_hub``: the names ``s3prl.hub.options()`` lists, every hubconf
entry of the served families with its signature, the reference's cache file names): ``register_into_s3prl`` installs our
entries without clobbering the reference's, and the hub-entry signatures / the expert attributes are what
``S3PRLUpstream.__init__`` (nn/upstream.py:102-140) uses."""

import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE_HUB = os.path.join(HERE, "golden", "reference_hub.json")


def _stand_in_s3prl(tmp_path):
    """A package ``s3prl`` whose ``hub`` module defines every name the reference's ``s3prl.hub.options()`` lists (placeholder
    callables) and an ``options()`` with the reference hub's rule (hub.py:40-54: the public callables of the module)."""
    ref = json.load(open(REFERENCE_HUB))
    pkg = tmp_path / "stand_in" / "s3prl"
    pkg.mkdir(parents=True)
    (pkg / "__init__.py").write_text("")
    body = ["def _placeholder(name):", "    def entry(*args, **kwargs):", "        raise NotImplementedError(name)",
            "    entry.__name__ = name", "    return entry", ""]
    body += [f"{name} = _placeholder({name!r})" for name in ref["options"]]
    body += ["", "def options(only_registered_ckpt=False):",
             "    suffixes = ('_local', '_url', '_gdriveid', '_custom')",
             "    return [n for n, v in list(globals().items()) if not n.startswith('_') and callable(v) and n != 'options'",
             "            and not (only_registered_ckpt and n.endswith(suffixes))]", ""]
    (pkg / "hub.py").write_text("\n".join(body))
    return str(tmp_path / "stand_in")


_SCRIPT = r"""
import inspect, json, os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[3])
ref = json.load(open(sys.argv[4]))
import s3prl.hub as ref_hub          # the stand-in of the reference hub: the names it lists
import s3prl_amd.hub as amd
from s3prl_amd.ckpt import save_checkpoint
from s3prl_amd.synth import named_config, synth_weights

assert sorted(ref_hub.options()) == ref["options"]
before = {n: getattr(ref_hub, n) for n in ref["options"]}
assert {"hubert_local", "wavlm_local", "wav2vec2_custom", "fbank"} <= set(before)
installed = amd.register_into_s3prl(prefix="amd_")
assert {"amd_hubert_local", "amd_distiller_local", "amd_unispeech_sat_local", "amd_wav2vec2_custom"} <= set(installed)
added = amd.register_into_s3prl()    # default: override=False -> same-named reference entries are left alone
for n, f in before.items():
    assert getattr(ref_hub, n) is f, n
assert set(added) == set(amd.options()) - set(before), sorted(set(added) ^ (set(amd.options()) - set(before)))
assert "amd_hubert_local" in ref_hub.options()
cfg = named_config("tiny_hubert")
path = os.path.join(sys.argv[2], "c.pt")
save_checkpoint(path, cfg, synth_weights(cfg, 0))
expert = getattr(ref_hub, "amd_hubert_local")(ckpt=path, refresh=False)
assert expert.get_downsample_rates("hidden_states") == 320
assert expert.num_layers == cfg.encoder_layers + 1 and expert.hidden_sizes == [cfg.encoder_embed_dim] * expert.num_layers
sigs = {name: params for entries in ref["hubconfs"].values() for name, params in entries}
for name in ("hubert_custom", "wav2vec2_custom"):   # hubert/hubconf.py:29-66, wav2vec2/hubconf.py:28-66
    ours = inspect.signature(getattr(amd, name))
    assert [k for k, _, _ in sigs[name]] == list(ours.parameters), name
    assert all(ours.parameters[k].default is False for k in ("legacy", "fairseq", "refresh"))
print("REFERENCE_HUB_OK")
"""


def test_register_into_the_real_hub_and_signatures(tmp_path):
    """Runs in a subprocess: the stand-in ``s3prl`` package and the registration stay out of the test process."""
    import subprocess

    root = os.path.dirname(HERE)
    out = subprocess.run([sys.executable, "-c", _SCRIPT, root, str(tmp_path), _stand_in_s3prl(tmp_path), REFERENCE_HUB],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "REFERENCE_HUB_OK" in out.stdout, out.stderr[-3000:]


_NAMES_SCRIPT = r"""
import inspect, json, os, sys
sys.path.insert(0, sys.argv[1])
ref = json.load(open(sys.argv[3]))
import s3prl_amd.hub as amd
checked = 0
for family, entries in ref["hubconfs"].items():
    for name, params in entries:
        assert name in ref["options"], name                        # it IS a name the reference hub serves
        assert hasattr(amd, name), f"{family}: s3prl_amd.hub lacks {name}"
        ours = inspect.signature(getattr(amd, name))
        assert [list(p) for p in params] == [[k, v.kind.name, repr(v.default)] for k, v in ours.parameters.items()], \
               (name, params, str(ours))
        assert name in amd.options(), name
        checked += 1
assert checked >= 60, checked
# the released names are not "_local / _url / _custom" entries: S3PRLUpstream.available_names(only_registered_ckpt=True)
reg = set(amd.options(only_registered_ckpt=True))
assert {"hubert_base", "hubert_large_ll60k", "wav2vec2_large_ll60k", "xls_r_300m", "wavlm_large", "wavlm_base_plus",
        "unispeech_sat_large", "data2vec_large_ll60k", "contentvec"} <= reg
assert all(n in ref["registered_ckpt_options"] for _, entries in ref["hubconfs"].items() for n, _ in entries if n in reg)
# cache naming rule = the reference's (util/download.py:186-208)
from s3prl_amd import download as our_dl
our_dl.set_dir(sys.argv[2])
urls = (amd.hubert_base.url, amd.wavlm_large.url, amd.xlsr_53.legacy_url)
assert set(urls) == set(ref["cache_file_names"])
for url in urls:
    want = os.path.join(os.path.realpath(sys.argv[2]), ref["cache_file_names"][url])
    assert our_dl.urls_to_filepaths(url, download=False) == want, url
print("REFERENCE_NAMES_OK", checked)
"""


def test_every_released_name_of_the_reference_hubconfs_exists_with_the_same_signature(tmp_path):
    """`-u hubert_large_ll60k`, `S3PRLUpstream("wavlm_large")`: how every SUPERB recipe names an upstream."""
    import subprocess

    root = os.path.dirname(HERE)
    out = subprocess.run([sys.executable, "-c", _NAMES_SCRIPT, root, str(tmp_path), REFERENCE_HUB], capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0 and "REFERENCE_NAMES_OK" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]


def test_custom_entry_rejects_legacy_plus_fairseq():
    import s3prl_amd.hub as amd

    with pytest.raises(AssertionError):
        amd.hubert_custom("x.pt", legacy=True, fairseq=True)  # same mutual exclusion as hubert/hubconf.py:36-41


def test_fairseq_layout_conversion(tmp_path):
    """``fairseq=True``: {"cfg": {"task", "model"}, "model"} -> the converted format, next to the source file."""
    import torch

    import s3prl_amd.hub as amd
    from s3prl_amd.synth import named_config, synth_weights

    cfg = named_config("tiny_hubert")
    sd = {k: torch.from_numpy(v) for k, v in synth_weights(cfg, 3).items()}
    model_cfg = dict(extractor_mode="default", encoder_layers=3, encoder_embed_dim=128, encoder_ffn_embed_dim=256,
                     encoder_attention_heads=2, conv_pos=16, conv_pos_groups=4, activation_fn="gelu",
                     conv_feature_layers=str([tuple(t) for t in cfg.conv_layers]))
    src = tmp_path / "fairseq_style.pt"
    torch.save({"cfg": {"task": {"normalize": False, "label_rate": 50.0}, "model": model_cfg}, "model": sd,
                "task_state": {"dictionaries": [["a", "b"]]}}, str(src))
    expert = amd.hubert_custom(str(src), fairseq=True)
    assert (tmp_path / "fairseq_style.converted.pt").is_file()
    assert expert.cfg.to_dict() == cfg.to_dict()


def test_fairseq_layout_conversion_of_an_omegaconf_container(tmp_path, monkeypatch):
    """Released fairseq checkpoints pickle ``cfg`` as an ``omegaconf.DictConfig`` (hubert/convert.py:22-40 reads it through
    fairseq).  ``omegaconf`` is not installed here, so a stand-in package with the two things the branch touches — a picklable
    container class and ``OmegaConf.to_container`` — exercises it: the converted checkpoint must equal the plain-dict one."""
    import sys

    import torch

    pkg = tmp_path / "fake_site" / "omegaconf"
    pkg.mkdir(parents=True)
    (pkg / "__init__.py").write_text(
        "class DictConfig:\n"
        "    def __init__(self, content):\n"
        "        self._content = {k: DictConfig(v) if isinstance(v, dict) else v for k, v in content.items()}\n"
        "    def __getitem__(self, k):\n"
        "        return self._content[k]\n"
        "class OmegaConf:\n"
        "    @staticmethod\n"
        "    def to_container(cfg):\n"
        "        return {k: OmegaConf.to_container(v) if isinstance(v, DictConfig) else v for k, v in cfg._content.items()}\n")
    monkeypatch.syspath_prepend(str(tmp_path / "fake_site"))
    sys.modules.pop("omegaconf", None)
    import omegaconf

    import s3prl_amd.hub as amd
    from s3prl_amd.synth import named_config, synth_weights

    try:
        cfg = named_config("tiny_hubert")
        sd = {k: torch.from_numpy(v) for k, v in synth_weights(cfg, 3).items()}
        model_cfg = dict(extractor_mode="default", encoder_layers=3, encoder_embed_dim=128, encoder_ffn_embed_dim=256,
                         encoder_attention_heads=2, conv_pos=16, conv_pos_groups=4, activation_fn="gelu",
                         conv_feature_layers=str([tuple(t) for t in cfg.conv_layers]))
        src = tmp_path / "fairseq_omegaconf.pt"
        torch.save({"cfg": omegaconf.DictConfig({"task": {"normalize": False, "label_rate": 50.0}, "model": model_cfg}), "model": sd,
                    "task_state": {"dictionaries": [["a", "b"]]}}, str(src))
        expert = amd.hubert_custom(str(src), fairseq=True)
        assert expert.cfg.to_dict() == cfg.to_dict()
        conv = torch.load(str(tmp_path / "fairseq_omegaconf.converted.pt"), map_location="cpu", weights_only=False)
        assert isinstance(conv["model_cfg"], dict) and conv["model_cfg"]["encoder_layers"] == 3
        assert conv["task_cfg"] == {"normalize": False, "label_rate": 50.0} and conv["dictionaries_symbols"] == [["a", "b"]]
    finally:
        sys.modules.pop("omegaconf", None)
