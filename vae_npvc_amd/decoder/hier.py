"""Voice conversion over a decode directory with the hierarchical model
(`model_type: vae_npvc_amd.model.vqvae2`): `decoder.basic.Decoder` with the
conversion step `model.convert((feat (1, mel, T), target (1, 1)))`, which takes
utterances of any length one at a time.  A recipe selects it with

    decoder_type: vae_npvc_amd.decoder.hier
"""
from .basic import Decoder as _Decoder


class Decoder(_Decoder):
    def decode_step(self, feat, spk):
        return self.model.convert((feat, spk))
