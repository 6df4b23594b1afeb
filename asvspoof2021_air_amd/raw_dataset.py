"""The reference's raw-waveform datasets (raw_dataset.py) over the corpus' own ``.flac`` files.

    ASVspoof2019Raw(access_type, path_to_database, path_to_protocol, part)      raw_dataset.py:31-69
    ASVspoof2021evalRaw(path_to_database)                                        raw_dataset.py:132-147

Constructor arguments, directory and protocol path rules (the ``eval`` protocol lives under the database), the LA / PA tag
tables and the item tuples are the reference's - with one difference: where the reference decodes the file on the host
(``torchaudio_load`` -> ``librosa.load`` / ``sf.read``, raw_dataset.py:20-28) and returns the (1, L) waveform, an item
here carries the file's COMPRESSED audio frames (a uint8 tensor, its STREAMINFO in ``.flac_info``), and ``collate_fn``
packs a batch of them for the device decoder:

    [bytes, byte_off, lengths, blocksize, start, *default_collate(meta)]

which passes through ``DevicePrefetcher`` unchanged; ``FlacDecoder.decode(bytes, byte_off, lengths, blocksize, Lcap)``
then yields the (B, Lcap) batch ``Trainer.step(pcm, labels, start=start, lengths=lengths)`` reads.  ``start`` holds the
crop offsets exactly as ``dataset._collate_ragged`` draws them.  ``waveform(idx)`` is the reference's item[0]: one file
decoded on the GPU to the (1, L) float tensor (sample / 32768: what a libsndfile float read returns).

The reference resamples anything that is not 16 kHz (``librosa.load(sr=16000)``); this path does not: such a file raises.
"""
import os

import numpy as np
import torch
from torch.utils.data import Dataset
from torch.utils.data.dataloader import default_collate

from . import flac
from .dataset import LABEL, TAG_LA19, TAG_PA19, find_files

SAMPLE_RATE = 16000


class _RawFlac(Dataset):
    """What the two classes share: compressed items, the packed batch, the one-file decode."""

    def _init_raw(self, feat_len, hop, bytes_round):
        self.feat_len, self.hop, self.bytes_round = int(feat_len), int(hop), int(bytes_round)
        self._decoder = None

    def _row(self, filepath):
        row, info = flac.FlacSource([filepath]).item(0)
        if info.sample_rate != SAMPLE_RATE:
            raise ValueError("%s: sample_rate = %d: the reference resamples to %d (librosa.load), this path does not"
                             % (filepath, info.sample_rate, SAMPLE_RATE))
        row.flac_info = info
        return row

    def collate_fn(self, samples):
        """[bytes, byte_off, lengths, blocksize, start, *default_collate(meta)]: ``flac.pack`` of the compressed rows,
        and per utterance longer than feat_len frames one ``np.random.randint(T - feat_len)`` in item order (0 otherwise) -
        the draws of ``dataset._collate_ragged`` (dataset.py:69 of the reference)."""
        packed = flac.pack([(smp[0], smp[0].flac_info) for smp in samples], self.bytes_round)
        start = np.zeros(len(samples), dtype=np.int32)
        for j, smp in enumerate(samples):
            T = 1 + int(smp[0].flac_info.total_samples) // self.hop
            if T > self.feat_len:
                start[j] = np.random.randint(T - self.feat_len)
        return list(packed) + [torch.from_numpy(start)] + default_collate([tuple(smp[1:]) for smp in samples])

    def waveform(self, idx, device="cuda"):
        """File ``idx`` decoded on the GPU: the reference's (1, L) float waveform.  Raises FlacError if it does not decode."""
        row = self[idx][0]
        if self._decoder is None or self._decoder.device != torch.device(device):
            self._decoder = flac.FlacDecoder(device, depth=1)
        by, off, ln, bs = flac.pack([(row, row.flac_info)], self.bytes_round)
        n = int(row.flac_info.total_samples)
        pcm, _ = self._decoder.decode(by.to(device), off, ln, bs, Lcap=n, dtype=torch.float32, check=True)
        return pcm.clone()


class ASVspoof2019Raw(_RawFlac):
    """raw_dataset.py:31-69.  Items: (flac_bytes, filename, tag, label) with the protocol's ``tag`` / ``label`` strings
    (``self.tag`` / ``self.label`` map them, as in the reference)."""

    def __init__(self, access_type, path_to_database, path_to_protocol, part="train", feat_len=750, hop=160,
                 bytes_round=65536):
        super().__init__()
        self.access_type, self.ptd, self.part = access_type, path_to_database, part
        self.path_to_audio = os.path.join(self.ptd, access_type, "ASVspoof2019_" + access_type + "_" + part + "/flac/")
        self.path_to_protocol = path_to_protocol
        protocol = os.path.join(path_to_protocol, "ASVspoof2019." + access_type + ".cm." + part + ".trl.txt")
        if part == "eval":  # raw_dataset.py:40-42: the eval protocol is read from the database tree
            protocol = os.path.join(self.ptd, access_type, "ASVspoof2019_" + access_type + "_cm_protocols/ASVspoof2019." +
                                    access_type + ".cm." + part + ".trl.txt")
        self.tag = dict(TAG_LA19) if access_type == "LA" else dict(TAG_PA19)
        self.label = dict(LABEL)
        with open(protocol, "r") as f:
            self.all_info = [info.strip().split() for info in f.readlines()]
        self._init_raw(feat_len, hop, bytes_round)

    def __len__(self):
        return len(self.all_info)

    def __getitem__(self, idx):
        speaker, filename, _, tag, label = self.all_info[idx]
        return self._row(os.path.join(self.path_to_audio, filename + ".flac")), filename, tag, label


class ASVspoof2021evalRaw(_RawFlac):
    """raw_dataset.py:132-147: every ``*.flac`` under the directory, sorted.  Items: (flac_bytes, filename)."""

    def __init__(self, path_to_database, feat_len=750, hop=160, bytes_round=65536):
        super().__init__()
        self.ptd = self.path_to_audio = path_to_database
        self.all_files = find_files(self.path_to_audio, ext="flac")
        self._init_raw(feat_len, hop, bytes_round)

    def __len__(self):
        return len(self.all_files)

    def __getitem__(self, idx):
        filepath = self.all_files[idx]
        return self._row(filepath), os.path.basename(filepath)[:-5]
