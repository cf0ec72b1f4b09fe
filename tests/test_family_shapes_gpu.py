"""The shape helpers of a handle of every family against recorded answers: s3enc_num_frames, s3enc_num_output_frames,
s3enc_valid_frames, s3enc_downsample_rate and s3enc_num_states (a refusal is recorded as its message).  No forward runs: the only
device work is the creation of one tiny handle per family.

``python tests/test_family_shapes_gpu.py OUT.json`` re-records ``tests/golden/family_shapes.json`` (done once, on an MI355X, from
the commit before the family table went in).
"""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "family_shapes.json")

CONFIGS = ["tiny_hubert", "tiny_wav2vec2", "tiny_wavlm", "tiny_distiller", "tiny_multires", "tiny_wav2vec", "tiny_cpc", "tiny_apc",
           "tiny_mockingjay", "tiny_decoar", "tiny_npc", "tiny_vggish", "tiny_byol_a", "tiny_mae_ast"]
SELECTIONS = [None, "fairseq_layers", "fairseq_layers_before_residual"]


def window_and_hop(cfg):
    """The fewest samples that make a first frame (example, segment, step) and the samples between two of them, from the
    configuration alone."""
    if cfg.family in ("apc", "decoar", "npc"):  # kaldi framing: whole windows only
        return cfg.conv_layers[0][1], cfg.conv_layers[0][2]
    if cfg.family == "mockingjay":  # centred STFT, hop 160: 1 + n // 160 frames once n > 200
        return 201, 160
    if cfg.family == "vggish":  # an example is example_frames whole windows
        _, win, shift = cfg.conv_layers[0]
        return win + (cfg.vg_example_frames - 1) * shift, cfg.vg_example_hop * shift
    if cfg.family == "mae_ast":  # a step is kt whole 25 ms / 10 ms frames
        return 400 + (cfg.ma_kt - 1) * 160, cfg.ma_kt * 160
    if cfg.family == "byol_a":  # a segment is window samples, the last one padded
        return cfg.conv_layers[0][1], cfg.conv_layers[0][2]
    pads = list(getattr(cfg, "conv_pads", None) or []) or [0] * len(cfg.conv_layers)  # the conv stacks (cpc: zero-padded)

    def frames(n):
        for (_, k, s), p in zip(cfg.conv_layers, pads):
            n = (n + 2 * p - k) // s + 1 if n > 0 and n + 2 * p >= k else 0
        return n

    hop = 1
    for _, _, s in cfg.conv_layers:
        hop *= s
    return next(n for n in range(1, 100000) if frames(n) >= 1), hop


def lengths_of(cfg):
    w, hop = window_and_hop(cfg)
    return sorted({0, 1, w - 1, w, w + 1, w + 2 * hop + hop // 3, w + 5 * hop + (2 * hop) // 3 + 1})


def answers(enc, lengths):
    from s3prl_amd._lib import S3EncError

    def states(sel):
        try:
            return enc.num_states(sel)
        except S3EncError as err:
            return str(err)

    return {"lengths": lengths,
            "num_frames": [enc.num_frames(n) for n in lengths],
            "num_output_frames": [enc.num_output_frames(n) for n in lengths],
            "valid_frames": {f"{l},{n}": enc.valid_frames(l, n) for n in lengths for l in lengths if l <= n},
            "downsample_rate": enc.downsample_rate(),
            "num_states": [states(sel) for sel in SELECTIONS]}


def handle(name):
    from s3prl_amd.encoder import HipEncoder
    from s3prl_amd.synth import named_config, synth_weights

    cfg = named_config(name)
    return cfg, HipEncoder(cfg, synth_weights(cfg, 0), dtype="fp32", device=0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", CONFIGS)
def test_shape_helpers_answer_as_recorded(name):
    with open(GOLDEN) as f:
        golden = json.load(f)[name]
    cfg, enc = handle(name)
    try:
        got = answers(enc, lengths_of(cfg))
    finally:
        enc.close()
    for key in golden:  # key by key: a failure names the helper
        assert got[key] == golden[key], key
    assert set(got) == set(golden)


if __name__ == "__main__":
    rec = {}
    for name in CONFIGS:
        cfg, enc = handle(name)
        lengths = lengths_of(cfg)
        rec[name] = answers(enc, lengths)
        enc.close()
        w = window_and_hop(cfg)[0]
        if cfg.family != "byol_a":  # (a BYOL-A segment is padded: one sample makes one)
            assert rec[name]["num_frames"][lengths.index(w - 1)] == 0 and rec[name]["num_frames"][lengths.index(w)] >= 1, name
    with open(sys.argv[1], "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"recorded {len(rec)} handles")
