"""Voice conversion over a decode directory with a hierarchical model
(`model_type: vae_npvc_amd.model.vqvae2`, `.vqvae2a` or `.vqvae2b`):
`decoder.basic.Decoder` with the
conversion step `model.convert((feat (1, mel, T), target (1, 1)))`, which takes
utterances of any length one at a time.  A recipe selects it with

    decoder_type: vae_npvc_amd.decoder.hier

`decode_batch_size: N` (default 1: the loop above, unchanged) converts up to N
trials per call as one padded batch, `model.convert((x, y), lengths=...)`; the
windowing, the batching by length and the writer are `decoder.basic`'s.
"""
from .basic import WINDOW_BATCHES  # noqa: F401  (the window is decoder.basic's)
from .basic import Decoder as _Decoder


class Decoder(_Decoder):
    batch_method = "convert"

    def decode_step(self, feat, spk):
        return self.model.convert((feat, spk))

    def decode_batch_step(self, x, y, lens):
        return self.model.convert((x, y), lengths=lens)
