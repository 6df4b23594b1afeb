"""The reference's raw-waveform datasets (raw_dataset.py) over the corpora's own ``.flac`` and ``.wav`` files.

    ASVspoof2019Raw(access_type, path_to_database, path_to_protocol, part)                   raw_dataset.py:31-69    flac
    VCC2020Raw(path_to_spoof, path_to_bonafide)                                               raw_dataset.py:72-98    wav
    ASVspoof2015Raw(path_to_database, path_to_protocol, part)                                 raw_dataset.py:101-129  wav
    ASVspoof2021evalRaw(path_to_database)                                                     raw_dataset.py:132-147  flac
    ASVspoof2019LARaw_withTransmission(path_to_database, path_to_protocol, part)              raw_dataset.py:149-184  wav
    ASVspoof2019LARaw_withTransmissionAndDevice(path_to_database, path_to_protocol, part)     raw_dataset.py:187-223  wav
    ASVspoof2019DFRaw_withCompression(path_to_database, path_to_protocol, part)               raw_dataset.py:226-261  wav
    ASVspoof2019DFRaw_withCompressionAndDevice(path_to_database, path_to_protocol, part)      raw_dataset.py:264-300  wav

Constructor argument names and order, directory and protocol path rules, the tag / label tables and the item tuples are
the reference's (its lab-local default paths are not: the path arguments are required) - with one difference: where the
reference decodes the file on the host (``torchaudio_load`` -> ``librosa.load(sr=16000)``, raw_dataset.py:20-28) and
returns the (1, L) waveform at 16 kHz, item 0 here carries the file's bytes as a uint8 tensor - the COMPRESSED audio
frames of a ``.flac`` (its STREAMINFO in ``.flac_info``), the ``data`` payload of a ``.wav`` (its header in
``.wav_info``) - and ``collate_fn`` packs a batch of them for the device:

    flac:  [bytes, byte_off, lengths, blocksize, start, *default_collate(meta)]
    wav:   [bytes, byte_off, frames, fmt, rate, lengths, start, *default_collate(meta)]

which passes through ``DevicePrefetcher`` unchanged (``rate`` is a tuple of host integers); ``FlacDecoder.decode(bytes,
byte_off, lengths, blocksize, Lcap)`` / ``WavDecoder.decode(bytes, byte_off, frames, fmt, rate, Lcap)`` then yield the
(B, Lcap) batch ``Trainer.step(pcm, labels, start=start, lengths=lengths)`` reads.  For ``.wav`` the decoder converts the
sample format, mixes down to mono and resamples any served rate to 16 kHz in the same launch (wav.py, resample.py);
``lengths`` are the OUTPUT lengths, computed from the headers on the host.  ``start`` holds the crop offsets exactly as
``dataset._collate_ragged`` draws them, from the length at 16 kHz.  ``waveform(idx)`` is the reference's item[0]: one
file decoded on the GPU to the (1, L) float tensor (what a libsndfile float read returns, at 16 kHz).

The FLAC classes refuse a file that is not at 16 kHz unless constructed with ``resample=True``; then the collate list is
``[bytes, byte_off, lengths, blocksize, start, rate, out_lengths, *meta]`` and the decode is ``FlacDecoder.decode``
followed by ``Resampler.resample(pcm, lengths, rate, Lcap)``.  The resampler is defined by its formulas (resample.py);
parity with ``librosa.load``'s own is not pinned.
"""
import os

import numpy as np
import torch
from torch.utils.data import Dataset
from torch.utils.data.dataloader import default_collate

from . import flac, resample, wav
from .dataset import LABEL, TAG_LA19, TAG_PA19, find_files

SAMPLE_RATE = 16000


def _draw_start(lengths, hop, feat_len):
    """Per utterance longer than feat_len frames one ``np.random.randint(T - feat_len)`` in item order (0 otherwise),
    T = 1 + length // hop: the draws of ``dataset._collate_ragged`` (dataset.py:69 of the reference)."""
    start = np.zeros(len(lengths), dtype=np.int32)
    for j, n in enumerate(lengths):
        T = 1 + int(n) // hop
        if T > feat_len:
            start[j] = np.random.randint(T - feat_len)
    return torch.from_numpy(start)


class _RawFlac(Dataset):
    """What the two FLAC classes share: compressed items, the packed batch, the one-file decode."""

    def _init_raw(self, feat_len, hop, bytes_round, resample=False):
        self.feat_len, self.hop, self.bytes_round = int(feat_len), int(hop), int(bytes_round)
        self.resample = bool(resample)
        self._decoder = self._resampler = None

    def _row(self, filepath):
        row, info = flac.FlacSource([filepath]).item(0)
        if info.sample_rate != SAMPLE_RATE:
            if not self.resample:
                raise ValueError("%s: sample_rate = %d: the reference resamples to %d (librosa.load), this path does not"
                                 % (filepath, info.sample_rate, SAMPLE_RATE))
            resample.geometry(info.sample_rate, SAMPLE_RATE, filepath)
        row.flac_info = info
        return row

    def collate_fn(self, samples):
        """[bytes, byte_off, lengths, blocksize, start, *default_collate(meta)]: ``flac.pack`` of the compressed rows and
        the crop draws of ``_draw_start``.  With ``resample=True``: [..., start, rate, out_lengths, *meta] - ``rate`` a
        tuple of the rows' rates in Hz, ``out_lengths`` the lengths at 16 kHz, which ``start`` is then drawn from."""
        infos = [smp[0].flac_info for smp in samples]
        packed = flac.pack([(smp[0], smp[0].flac_info) for smp in samples], self.bytes_round)
        meta = default_collate([tuple(smp[1:]) for smp in samples])
        if not self.resample:
            return list(packed) + [_draw_start([i.total_samples for i in infos], self.hop, self.feat_len)] + meta
        rate = tuple(int(i.sample_rate) for i in infos)
        resample.distinct(rate)
        out = [resample.out_length(int(i.total_samples), int(i.sample_rate), SAMPLE_RATE) for i in infos]
        return list(packed) + [_draw_start(out, self.hop, self.feat_len), rate, torch.tensor(out, dtype=torch.int32)] + meta

    def waveform(self, idx, device="cuda"):
        """File ``idx`` decoded on the GPU: the reference's (1, L) float waveform.  Raises FlacError if it does not decode."""
        row = self[idx][0]
        if self._decoder is None or self._decoder.device != torch.device(device):
            self._decoder = flac.FlacDecoder(device, depth=1)
            self._resampler = None
        by, off, ln, bs = flac.pack([(row, row.flac_info)], self.bytes_round)
        n, sr = int(row.flac_info.total_samples), int(row.flac_info.sample_rate)
        if sr == SAMPLE_RATE:
            pcm, _ = self._decoder.decode(by.to(device), off, ln, bs, Lcap=n, dtype=torch.float32, check=True)
            return pcm.clone()
        if self._resampler is None:
            self._resampler = resample.Resampler(device, depth=1)
        pcm, _ = self._decoder.decode(by.to(device), off, ln, bs, Lcap=n, dtype=torch.int16, check=True)
        y, _ = self._resampler.resample(pcm, ln, (sr,), Lcap=resample.out_length(n, sr, SAMPLE_RATE), check=True)
        return y.clone()


class ASVspoof2019Raw(_RawFlac):
    """raw_dataset.py:31-69.  Items: (flac_bytes, filename, tag, label) with the protocol's ``tag`` / ``label`` strings
    (``self.tag`` / ``self.label`` map them, as in the reference)."""

    def __init__(self, access_type, path_to_database, path_to_protocol, part="train", feat_len=750, hop=160,
                 bytes_round=65536, resample=False):
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
        self._init_raw(feat_len, hop, bytes_round, resample)

    def __len__(self):
        return len(self.all_info)

    def __getitem__(self, idx):
        speaker, filename, _, tag, label = self.all_info[idx]
        return self._row(os.path.join(self.path_to_audio, filename + ".flac")), filename, tag, label


class ASVspoof2021evalRaw(_RawFlac):
    """raw_dataset.py:132-147: every ``*.flac`` under the directory, sorted.  Items: (flac_bytes, filename)."""

    def __init__(self, path_to_database, feat_len=750, hop=160, bytes_round=65536, resample=False):
        super().__init__()
        self.ptd = self.path_to_audio = path_to_database
        self.all_files = find_files(self.path_to_audio, ext="flac")
        self._init_raw(feat_len, hop, bytes_round, resample)

    def __len__(self):
        return len(self.all_files)

    def __getitem__(self, idx):
        filepath = self.all_files[idx]
        return self._row(filepath), os.path.basename(filepath)[:-5]


# ------------------------------------------------------------------------------------------------ the .wav classes
TAG_2015 = dict([("human", 0)] + [("S%d" % i, i) for i in range(1, 11)])  # raw_dataset.py:110-111
LABEL_2015 = {"spoof": 1, "human": 0}                                     # raw_dataset.py:112
TAG_AUG19 = dict([("-", 0)] + [("A%02d" % i, i) for i in range(1, 8)])    # raw_dataset.py:161


class _RawWav(Dataset):
    """What the six WAV classes share: payload items, the packed batch, the one-file decode."""

    def _init_raw(self, feat_len, hop, bytes_round, target_sr=SAMPLE_RATE):
        self.feat_len, self.hop, self.bytes_round, self.target_sr = int(feat_len), int(hop), int(bytes_round), int(target_sr)
        self._decoder = None

    def _row(self, filepath):
        row, info = wav.WavSource([filepath], self.target_sr).item(0)
        row.wav_info = info
        return row

    def collate_fn(self, samples):
        """[bytes, byte_off, frames, fmt, rate, lengths, start, *default_collate(meta)]: ``wav.pack`` of the payload rows
        and the crop draws of ``_draw_start`` over the OUTPUT lengths."""
        packed = wav.pack([(smp[0], smp[0].wav_info) for smp in samples], self.bytes_round, self.target_sr)
        start = _draw_start(packed[5].tolist(), self.hop, self.feat_len)
        return list(packed) + [start] + default_collate([tuple(smp[1:]) for smp in samples])

    def waveform(self, idx, device="cuda"):
        """File ``idx`` converted on the GPU: the reference's (1, L) float waveform at 16 kHz."""
        row = self[idx][0]
        if self._decoder is None or self._decoder.device != torch.device(device):
            self._decoder = wav.WavDecoder(device, depth=1, target_sr=self.target_sr)
        by, off, fr, fm, rate, ln = wav.pack([(row, row.wav_info)], self.bytes_round, self.target_sr)
        pcm, _ = self._decoder.decode(by.to(device), off, fr, fm, rate, Lcap=int(ln[0]), dtype=torch.float32, check=True)
        return pcm.clone()


class VCC2020Raw(_RawWav):
    """raw_dataset.py:72-98: every ``*.wav`` under the two trees, bona fide first.  Items: (wav_bytes, filename, tag,
    label) - bona fide: the last three path components joined by ``_``, tag ``-``; spoof: the base name, the tag is the
    directory two levels up."""

    def __init__(self, path_to_spoof, path_to_bonafide, feat_len=750, hop=160, bytes_round=65536):
        super().__init__()
        self.all_spoof = find_files(path_to_spoof, ext="wav")
        self.all_bonafide = find_files(path_to_bonafide, ext="wav")
        self._init_raw(feat_len, hop, bytes_round)

    def __len__(self):
        return len(self.all_spoof) + len(self.all_bonafide)

    def __getitem__(self, idx):
        if idx < len(self.all_bonafide):
            filepath = self.all_bonafide[idx]
            label = "bonafide"
            filename = "_".join(filepath.split("/")[-3:])[:-4]
            tag = "-"
        else:
            filepath = self.all_spoof[idx - len(self.all_bonafide)]
            filename = os.path.basename(filepath)[:-4]
            label = "spoof"
            tag = filepath.split("/")[-3]
        return self._row(filepath), filename, tag, label


class ASVspoof2015Raw(_RawWav):
    """raw_dataset.py:101-129.  Items: (wav_bytes, filename with ``_`` -> ``-``, tag, label) in protocol order; the file
    is <database>/<part>/<speaker>/<filename>.wav."""

    def __init__(self, path_to_database, path_to_protocol, part="train", feat_len=750, hop=160, bytes_round=65536):
        super().__init__()
        self.ptd, self.part = path_to_database, part
        self.path_to_audio = os.path.join(self.ptd, self.part)
        self.path_to_protocol = path_to_protocol
        cm_pro_dict = {"train": "cm_train.trn", "dev": "cm_develop.ndx", "eval": "cm_evaluation.ndx"}
        protocol = os.path.join(self.path_to_protocol, cm_pro_dict[self.part])
        self.tag, self.label = dict(TAG_2015), dict(LABEL_2015)
        with open(protocol, "r") as f:
            self.all_info = [info.strip().split() for info in f.readlines()]
        self._init_raw(feat_len, hop, bytes_round)

    def __len__(self):
        return len(self.all_info)

    def __getitem__(self, idx):
        speaker, filename, tag, label = self.all_info[idx]
        row = self._row(os.path.join(self.path_to_audio, speaker, filename + ".wav"))
        return row, filename.replace("_", "-"), tag, label


class _Aug19Raw(_RawWav):
    """The four augmented ASVspoof 2019 sets (raw_dataset.py:149-300): every ``*.wav`` under <database>/<part>, sorted; the
    base name is <protocol file name>_<channel>[_<device>]; speaker, tag and label come from the LA protocol (for
    ``eval`` read from <database>/LA/ASVspoof2019_LA_cm_protocols/)."""

    FIELDS = 1  # trailing ``_`` fields of the base name: channel [, device]

    def __init__(self, path_to_database, path_to_protocol, part="train", feat_len=750, hop=160, bytes_round=65536):
        super().__init__()
        self.ptd, self.part = path_to_database, part
        self.path_to_audio = os.path.join(self.ptd, self.part)
        self.path_to_protocol = path_to_protocol
        protocol = os.path.join(self.path_to_protocol, "ASVspoof2019.LA.cm." + self.part + ".trl.txt")
        if self.part == "eval":
            protocol = os.path.join(self.ptd, "LA", "ASVspoof2019_LA_cm_protocols/ASVspoof2019.LA.cm." + self.part + ".trl.txt")
        self.tag, self.label = dict(TAG_AUG19), dict(LABEL)
        self.all_files = find_files(self.path_to_audio, ext="wav")
        self.all_info = {}
        with open(protocol, "r") as f:
            for info in f.readlines():
                speaker, filename, _, tag, label = info.strip().split()
                self.all_info[filename] = (speaker, tag, label)
        self._init_raw(feat_len, hop, bytes_round)

    def __len__(self):
        return len(self.all_files)

    def __getitem__(self, idx):
        filepath = self.all_files[idx]
        fields = os.path.basename(filepath)[:-4].split("_")
        filename = "_".join(fields[:-self.FIELDS])
        speaker, tag, label = self.all_info[filename]
        return (self._row(filepath), filename, tag, label) + tuple(fields[-self.FIELDS:])


class ASVspoof2019LARaw_withTransmission(_Aug19Raw):
    """raw_dataset.py:149-184.  Items: (wav_bytes, filename, tag, label, channel)."""


class ASVspoof2019LARaw_withTransmissionAndDevice(_Aug19Raw):
    """raw_dataset.py:187-223.  Items: (wav_bytes, filename, tag, label, channel, device)."""
    FIELDS = 2


class ASVspoof2019DFRaw_withCompression(_Aug19Raw):
    """raw_dataset.py:226-261.  Items: (wav_bytes, filename, tag, label, channel)."""


class ASVspoof2019DFRaw_withCompressionAndDevice(_Aug19Raw):
    """raw_dataset.py:264-300.  Items: (wav_bytes, filename, tag, label, channel, device)."""
    FIELDS = 2
