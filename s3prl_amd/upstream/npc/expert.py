"""MI355X-native stand-in for ``s3prl/upstream/npc/expert.py::UpstreamExpert`` (same constructor / forward / get_downsample_rates
contract; the forward runs in libs3enc's HIP kernels, csrc/npc.hip, csrc/fbank.hip and csrc/convtaps.hip).

``forward(wavs)`` returns what ``UpstreamBase.__call__`` builds from the reference's hooks (npc/expert.py:28-41) in the order they
fire: ``blocks[0]``, ``masked_convs[0]``, ``blocks[1]``, ``masked_convs[1]``, ..., and ``self.model``'s ``output[1]``, the sum of
the masked outputs — ``2 n_blocks + 1`` states.  With ``disable_cross_layer`` the hooks on the ``None`` entries never fire: the
blocks, the last masked conv, and that tensor again as the last state (``n_blocks + 2``).  The reference's forward returns nothing
itself, so there is no ``default`` key.

Unlike APC there is NO length masking: the reference convolves all ``T`` rows of the padded batch, so the rows behind an
utterance's own frames are the reference's (loud) values, not zeros, and an utterance's rows depend on the batch's ``T``.  The
quantizer and the post-net feed only the prediction that the upstream discards."""

from ..base import HipUpstreamExpert


class UpstreamExpert(HipUpstreamExpert):
    family = "npc"

    def get_downsample_rates(self, key: str = None) -> int:
        return 160  # npc/expert.py:43-44

    def _states_info(self, n: int):
        c, names = self.cfg, []
        for i in range(c.npc_blocks):
            names.append(f"self.model.blocks[{i}]")
            if c.npc_has_mask(i):
                names.append(f"self.model.masked_convs[{i}]")
        return tuple(names) + ("self.model",)
