"""A synthetic Kaldi data directory for the resident-corpus tests: a dozen
utterances of 24 mel, 3 to 90 frames, so that with crop 32 several are shorter
than the crop, some equal it and the rest draw a random start."""
import numpy as np

from vae_npvc_amd.dataset import kaldi_io as K

MEL, CROP = 24, 32
LENGTHS = [3, 90, 32, 31, 33, 64, 17, 45, 8, 70, 32, 57]
CFG = {"crop_length": CROP}


def make_data_dir(root, lengths=LENGTHS, mel=MEL, compression=None, seed=5):
    """feats.ark/.scp, utt2num_frames, utt2spk_id under `root`; returns the matrices in item order."""
    rng = np.random.default_rng(seed)
    mats = []
    with K.WriteHelper(f"ark,scp:{root}/feats.ark,{root}/feats.scp", compression_method=compression) as w:
        for i, n in enumerate(lengths):
            mats.append(rng.standard_normal((n, mel)).astype(np.float32))
            w[f"spk{i % 5}_utt{i}"] = mats[-1]
    with open(root / "utt2num_frames", "w") as f:
        for i, n in enumerate(lengths):
            f.write(f"spk{i % 5}_utt{i} {n}\n")
    with open(root / "utt2spk_id", "w") as f:
        for i in range(len(lengths)):
            f.write(f"spk{i % 5}_utt{i} {(i * 7) % 5 + 11}\n")
    return mats
