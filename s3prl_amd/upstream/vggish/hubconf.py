"""hub entry of VGGish under the reference's name and signature (s3prl/upstream/vggish/hubconf.py:34-42): ``vggish(*args,
**kwargs)``.  Its two URLs — the model and the PCA parameters — resolve to the reference's cache files (``s3prl_amd.download``)
and are handed to the expert as the dict ``{"vggish": ..., "pca": ...}``."""

from ...download import urls_to_filepaths as _urls_to_filepaths
from .expert import UpstreamExpert as _UpstreamExpert


def _load_state_dict_from_url(url):
    import torch

    return torch.load(_urls_to_filepaths(url), map_location="cpu", weights_only=False)


def _vggish_from_torch_hub(urls, *args, **kwargs):
    kwargs["ckpt"] = {
        "vggish": _load_state_dict_from_url(urls["vggish"]),
        "pca": _load_state_dict_from_url(urls["pca"]),
    }
    return _UpstreamExpert(*args, **kwargs)


def vggish(*args, **kwargs):
    urls = {
        "vggish": "https://github.com/harritaylor/torchvggish/releases/download/v0.1/vggish-10086976.pth",
        "pca": "https://github.com/harritaylor/torchvggish/releases/download/v0.1/vggish_pca_params-970ea276.pth",
    }
    return _vggish_from_torch_hub(urls, *args, **kwargs)
