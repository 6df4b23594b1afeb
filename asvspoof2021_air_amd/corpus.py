"""The decoded corpus in HBM, and the batch selection of main_train.py:226-345 on the device.

``DeviceCorpus`` holds every utterance of a training set once, decoded, in one flat int16 or float32 device tensor
(the 25,380 utterances of the 2019 LA training partition are at most 10.6 GB as int16), with its lengths, labels,
tags, indices and ``--ADV_AUG`` channel ids beside it.  ``DeviceCorpus.from_dataset`` fills it in one pass over a
dataset the package already reads; ``corpus.sampler(...)`` then yields ragged training batches as device tensors -
permutation, mixing of the two flows, crop draw and gather all run on the device, so an epoch costs no decode, no
collate function, no pinned ring and no host synchronisation:

    corpus = DeviceCorpus.from_dataset(ASVspoof2019Raw("LA", database, protocol, "train"))
    sampler = corpus.sampler(64, seed=688)
    for epoch_num in range(200):
        trainer.train_epoch(sampler.epoch(), epoch_num)

What is host code here (``Schedule``, ``resolve_lcap``) runs without a GPU: which rows of which permutation form the
next batch follows from a few integers.  The random words, the key layout and the crop rule are documented at
include/air_hip.h, "device corpus", and restated in tests/corpus_oracle.py.
"""
import collections

import numpy as np
import torch

from . import ops
from .ragged import RAGGED_ROUND, PinnedUpload, round_capacity  # noqa: F401  (RAGGED_ROUND: re-exported)

MAX_PERMUTATION = 1 << 20       # air_eval_max_trials(): the longest range one flow permutes

DeviceBatch = collections.namedtuple("DeviceBatch", ("pcm", "labels", "start", "lengths", "tags", "channels", "index"))


def _round_up(n, m):
    return -(-int(n) // m) * m


# ---------------------------------------------------------------------------------------------- host: the schedule
class Schedule:
    """Which rows of which permutation form each batch - the two SubsetRandomSamplers and the restarting iterator of
    main_train.py:226-345 as a few integers.  ``ranges``: one or two (lo, hi) index ranges, the flows.  Two flows need
    ``ratio``: rows 0 .. int(B * ratio) - 1 of every batch come from the first, the rest from the second.  An epoch is
    as many steps as the first flow gives; it is re-permuted at every epoch start (generation = the epoch's number).
    The second flow keeps its cursor across epochs and takes a new generation whenever fewer rows remain than a step
    of all ranks needs.  At global step s rank k draws rows [(s * world + k) * b, +b) of a flow's permutation: every
    rank derives the same permutations and no two share a row.

    ``next_step()`` returns the step's segments ``[(flow, generation, first, count), ...]`` for this rank."""

    def __init__(self, ranges, batch_size, ratio=None, shuffle=True, drop_last=None, rank=0, world=1):
        self.ranges = [(int(lo), int(hi)) for lo, hi in ranges]
        self.batch_size, self.shuffle = int(batch_size), bool(shuffle)
        self.drop_last = self.shuffle if drop_last is None else bool(drop_last)
        self.rank, self.world = int(rank), int(world)
        if len(self.ranges) not in (1, 2):
            raise ValueError("ranges holds one or two (lo, hi) pairs, got %d" % len(self.ranges))
        for lo, hi in self.ranges:
            if lo < 0 or hi <= lo:
                raise ValueError("empty or negative range (%d, %d)" % (lo, hi))
            if self.shuffle and hi - lo > MAX_PERMUTATION:
                raise ValueError("a flow permutes at most %d utterances, the range (%d, %d) has %d" % (
                    MAX_PERMUTATION, lo, hi, hi - lo))
        if self.batch_size < 1:
            raise ValueError("batch_size must be positive")
        if self.world < 1 or not 0 <= self.rank < self.world:
            raise ValueError("rank %d of world %d" % (self.rank, self.world))
        if len(self.ranges) == 2:
            if ratio is None or not self.shuffle:
                raise ValueError("two ranges are the reference's two shuffled flows: give ratio, keep shuffle")
            b0 = int(self.batch_size * ratio)  # main_train.py:226
            self.rows = (b0, self.batch_size - b0)
            if b0 < 1 or self.rows[1] < 1:
                raise ValueError("batch_size %d at ratio %r leaves a flow without rows" % (self.batch_size, ratio))
            if self.sizes[1] < self.world * self.rows[1]:
                raise ValueError("the second range has %d utterances, one step needs %d" % (
                    self.sizes[1], self.world * self.rows[1]))
        else:
            if ratio is not None:
                raise ValueError("ratio mixes two ranges")
            self.rows = (self.batch_size,)
        per = self.world * self.rows[0]
        self.steps = self.sizes[0] // per if self.drop_last else -(-self.sizes[0] // per)
        self.epochs = 0                        # epochs begun
        self.step = self.steps                 # position inside the current epoch (none begun: at its end)
        self.generation = [0] * len(self.ranges)
        self.cursor = [0] * len(self.ranges)   # rows of the flow's permutation taken so far, over all ranks

    @property
    def sizes(self):
        return [hi - lo for lo, hi in self.ranges]

    def __len__(self):
        return self.steps

    def begin_epoch(self):
        self.generation[0] = self.epochs
        self.cursor[0] = 0
        self.epochs += 1
        self.step = 0

    def next_step(self):
        """The next step's segments, or None at the end of the epoch."""
        if self.step >= self.steps:
            return None
        self.step += 1
        segs = []
        for f, b in enumerate(self.rows):
            n, take = self.sizes[f], self.world * b
            if f == 1 and n - self.cursor[1] < take:  # main_train.py:317-321: the iterator is restarted
                self.generation[1] += 1
                self.cursor[1] = 0
            first = self.cursor[f] + self.rank * b
            segs.append((f, self.generation[f], first, max(0, min(b, n - first))))
            self.cursor[f] += take
        return segs

    def state_dict(self):
        return {"epochs": self.epochs, "step": self.step, "generation": list(self.generation), "cursor": list(self.cursor)}

    def load_state_dict(self, state):
        if len(state["generation"]) != len(self.ranges) or len(state["cursor"]) != len(self.ranges):
            raise ValueError("the state is of %d flows, the schedule has %d" % (len(state["generation"]), len(self.ranges)))
        self.epochs, self.step = int(state["epochs"]), int(state["step"])
        self.generation = [int(g) for g in state["generation"]]
        self.cursor = [int(c) for c in state["cursor"]]


def resolve_lcap(Lcap, lengths, ranges):
    """The batch capacity: ``Lcap`` checked against the utterances of ``ranges`` (``lengths``: the host's copy), or its
    default, their longest rounded up to RAGGED_ROUND."""
    lengths = np.asarray(lengths)
    longest = max(int(lengths[lo:hi].max()) for lo, hi in ranges)
    if Lcap is None:
        return round_capacity(longest)
    Lcap = int(Lcap)
    if Lcap < ops.CORPUS_ALIGN or Lcap % ops.CORPUS_ALIGN:
        raise ValueError("Lcap must be a positive multiple of %d, got %d" % (ops.CORPUS_ALIGN, Lcap))
    if Lcap < longest:
        raise ValueError("Lcap = %d, the longest utterance of the ranges has %d samples" % (Lcap, longest))
    return Lcap


# ---------------------------------------------------------------------------------------------- device: the store
class DeviceCorpus:
    """A flat device store of utterances.  ``samples``: 1-d int16 | float32, utterance i at
    ``samples[offsets[i] : offsets[i] + lengths[i]]``, every offset a multiple of 8 elements (16-byte rows for the
    copy kernels; what lies in the gaps is never read as data).  Tables, all on the device: ``offsets`` int64 (N + 1),
    ``lengths`` int32, ``labels`` / ``tags`` / ``index`` int64 (N), ``channels`` int64 (N, C) or None.  The host keeps
    the lengths too (``host_lengths``): they arrive on the host, and everything the host must decide - offsets, grid
    sizes, capacities - follows from them without reading device memory."""

    def __init__(self, dtype=torch.int16, device="cuda"):
        if dtype not in ops.CORPUS_DTYPES:
            raise ValueError("a corpus is torch.int16 or torch.float32, got %s" % (dtype,))
        self.dtype, self.device = dtype, torch.device(device)
        if self.device.type != "cuda":
            raise ops._hip.AirError("DeviceCorpus lives on the GPU (the HIP path has no CPU fallback)")
        self.n = 0
        self._end = 0                  # first free element of the store (a multiple of 8)
        self._host_lengths = []
        self._samples = None
        self._tables = None            # name -> tensor of capacity ``_ucap`` rows (offsets: + 1)
        self._ucap = 0
        self.n_channels = None         # fixed by the first append: 0 = none
        self._upload = PinnedUpload()

    # -- views
    def __len__(self):
        return self.n

    @property
    def host_lengths(self):
        return np.asarray(self._host_lengths, dtype=np.int64)

    @property
    def samples(self):
        return self._samples[:self._end] if self._samples is not None else torch.empty(0, dtype=self.dtype, device=self.device)

    def _table(self, name):
        if self._tables is None:
            raise ValueError("the corpus is empty")
        return self._tables[name]

    offsets = property(lambda self: self._table("offsets")[:self.n + 1])
    lengths = property(lambda self: self._table("lengths")[:self.n])
    labels = property(lambda self: self._table("labels")[:self.n])
    tags = property(lambda self: self._table("tags")[:self.n])
    index = property(lambda self: self._table("index")[:self.n])

    @property
    def channels(self):
        return self._table("channels")[:self.n] if self.n_channels else None

    @property
    def sample_bytes(self):
        """Bytes of the store in use, alignment gaps included."""
        return self._end * torch.empty(0, dtype=self.dtype).element_size()

    def bytes_per_hour(self, sample_rate=16000):
        """Store bytes per hour of audio held."""
        return self.sample_bytes / (float(sum(self._host_lengths)) / sample_rate / 3600.0)

    # -- capacity
    def reserve(self, samples, utterances):
        """Size the store for ``samples`` elements (gaps included: allow 7 per utterance) and ``utterances`` rows up
        front; appends beyond it grow by doubling through device-side copies."""
        self._reserve_samples(int(samples), exact=True)
        self._reserve_utterances(int(utterances), exact=True)
        return self

    def _reserve_samples(self, need, exact=False):
        have = self._samples.numel() if self._samples is not None else 0
        if need <= have:
            return
        grown = torch.empty(need if exact else max(need, 2 * have), dtype=self.dtype, device=self.device)
        if self._end:
            grown[:self._end].copy_(self._samples[:self._end])
        self._samples = grown

    def _reserve_utterances(self, need, exact=False):
        if need <= self._ucap and self._tables is not None:
            return
        cap = max(need, 1) if exact else max(need, 2 * self._ucap, 64)
        dev = self.device
        new = {"offsets": torch.empty(cap + 1, dtype=torch.int64, device=dev),
               "lengths": torch.empty(cap, dtype=torch.int32, device=dev)}
        for name in ("labels", "tags", "index"):
            new[name] = torch.empty(cap, dtype=torch.int64, device=dev)
        if self.n_channels:
            new["channels"] = torch.empty((cap, self.n_channels), dtype=torch.int64, device=dev)
        if self._tables is not None and self.n:
            for name, t in new.items():
                rows = self.n + 1 if name == "offsets" else self.n
                t[:rows].copy_(self._tables[name][:rows])
        self._tables, self._ucap = new, cap

    # -- filling
    def append(self, pcm, lengths, labels, tags=None, channels=None):
        """Pack the rows of a ragged (B, Lcap) device batch - what FlacDecoder.decode, WavDecoder.decode and the
        upload of ``_collate_ragged``'s batch give - behind what is held: one HIP launch.  ``lengths`` are HOST
        integers (the headers carry them), so the offsets are computed here and nothing synchronises.  ``labels``,
        ``tags`` (default 0) and ``channels`` ((B,) or (B, C) class ids; every append alike) may live on either
        side.  Returns the index of the first utterance appended."""
        if not torch.is_tensor(pcm) or not pcm.is_cuda or pcm.dim() != 2 or pcm.dtype != self.dtype:
            raise ValueError("pcm must be a (B, Lcap) %s tensor on the GPU" % (self.dtype,))
        if torch.is_tensor(lengths):
            if lengths.is_cuda:
                raise ValueError("lengths are given on the host (the offsets are computed there)")
            lengths = lengths.numpy()
        lens = np.asarray(lengths).reshape(-1).astype(np.int64)
        B, Lsrc = int(pcm.shape[0]), int(pcm.shape[1])
        if lens.size != B or B < 1 or int(lens.min()) < 1 or int(lens.max()) > Lsrc:
            raise ValueError("lengths must be %d integers in [1, %d]" % (B, Lsrc))
        dev, first = self.device, self.n
        meta = {"labels": labels, "tags": tags if tags is not None else torch.zeros(B, dtype=torch.int64)}
        for name, t in meta.items():
            t = torch.as_tensor(t).reshape(-1)
            if t.numel() != B or t.is_floating_point():
                raise ValueError("%s must be %d integers" % (name, B))
            meta[name] = t
        C = 0
        if channels is not None:
            channels = torch.as_tensor(channels).reshape(B, -1)
            C = int(channels.shape[1])
        if self.n_channels is None:
            self.n_channels = C
        elif self.n_channels != C:
            raise ValueError("this corpus holds %d channel ids per utterance, the batch gives %d" % (self.n_channels, C))
        pos = np.empty(B + 1, dtype=np.int64)
        pos[0] = self._end
        np.cumsum(_round_up_array(lens), out=pos[1:])
        pos[1:] += self._end
        self._reserve_samples(int(pos[B]))
        self._reserve_utterances(first + B)
        # one pinned upload for what the host computed: [offsets (B + 1) | lengths (B) | index (B)]
        pack = self._upload(np.concatenate((pos, lens, np.arange(first, first + B, dtype=np.int64))), dev)
        t = self._tables
        t["offsets"][first:first + B + 1].copy_(pack[:B + 1])
        t["lengths"][first:first + B].copy_(pack[B + 1:2 * B + 1])
        t["index"][first:first + B].copy_(pack[2 * B + 1:])
        for name in ("labels", "tags"):
            t[name][first:first + B].copy_(meta[name].to(torch.int64), non_blocking=True)
        if C:
            t["channels"][first:first + B].copy_(channels.to(torch.int64), non_blocking=True)
        ops.corpus_copy_rows(pcm.contiguous(), self._samples, t["lengths"][first:first + B], int(lens.max()),
                             src_stride=Lsrc, dst_off=t["offsets"][first:first + B])
        self._host_lengths.extend(int(v) for v in lens)
        self.n, self._end = first + B, int(pos[B])
        return first

    def row(self, i):
        """Utterance ``i`` as a view of the store."""
        if not 0 <= i < self.n:
            raise IndexError(i)
        off = int(np.sum(_round_up_array(self.host_lengths[:i])))
        return self._samples[off:off + self._host_lengths[i]]

    @classmethod
    def from_dataset(cls, ds, batch_size=64, dtype=torch.int16, device="cuda"):
        """The store of every utterance of ``ds`` in one pass: the FLAC and WAV classes of raw_dataset.py through their
        own ``collate_fn`` and decoder (one ``flac.check`` / ``wav.check`` over all rows at the end), the ``PCMSource``
        datasets of dataset.py with ``return_pcm='ragged'`` through theirs (their waveforms must be of ``dtype``).
        Labels and tags are the integers the dataset maps them to (-1 / 0 for an unlabelled set); the channel ids of
        the ``*_aug`` datasets become ``channels``.  The crop offsets the collate functions draw are dropped: the
        sampler draws its own."""
        from . import flac, raw_dataset, resample, wav
        from .dataset import _SpoofDataset
        from .devbuf import DeviceVector
        corpus = cls(dtype, device)
        dev = corpus.device
        n = len(ds)
        if isinstance(ds, raw_dataset._RawFlac):
            kind, dec = "flac", flac.FlacDecoder(dev)
            res = resample.Resampler(dev) if ds.resample else None
        elif isinstance(ds, raw_dataset._RawWav):
            kind, dec = "wav", wav.WavDecoder(dev, target_sr=ds.target_sr)
        elif isinstance(ds, _SpoofDataset) and ds.return_pcm == "ragged":
            kind = "pcm"
        else:
            raise ValueError("from_dataset reads the FLAC / WAV classes of raw_dataset.py and the dataset.py classes with "
                             "return_pcm='ragged', got %s" % type(ds).__name__)
        status = DeviceVector(torch.int32, dev, n)
        status2 = DeviceVector(torch.int32, dev, n)
        for lo in range(0, n, int(batch_size)):
            batch = ds.collate_fn([ds[i] for i in range(lo, min(n, lo + int(batch_size)))])
            if kind == "flac":
                by, off, ln, bs = batch[:4]
                meta = batch[(7 if ds.resample else 5):]
                cap = _round_up(int(ln.max()), ops.CORPUS_ALIGN)
                lens = ln
                if ds.resample:
                    rate, lens = batch[5], batch[6]
                    raw, st = dec.decode(by.to(dev, non_blocking=True), off, ln, bs, Lcap=cap, dtype=torch.int16)
                    pcm = torch.empty((len(ln), _round_up(int(lens.max()), ops.CORPUS_ALIGN)), dtype=dtype, device=dev)
                    res.resample(raw, ln, rate, Lcap=pcm.shape[1], dtype=dtype, out=pcm)
                    status2.append(res.last_status)
                else:
                    pcm = torch.empty((len(ln), cap), dtype=dtype, device=dev)
                    _, st = dec.decode(by.to(dev, non_blocking=True), off, ln, bs, Lcap=cap, dtype=dtype, out=pcm)
                status.append(st)
            elif kind == "wav":
                by, off, fr, fm, rate, lens = batch[:6]
                meta = batch[7:]
                pcm = torch.empty((len(lens), _round_up(int(lens.max()), ops.CORPUS_ALIGN)), dtype=dtype, device=dev)
                _, st = dec.decode(by.to(dev, non_blocking=True), off, fr, fm, rate, Lcap=pcm.shape[1], dtype=dtype, out=pcm)
                status.append(st)
            else:
                pcm, lens = batch[0], batch[1]
                meta = batch[3:]
                if pcm.dtype != dtype:
                    raise ValueError("the dataset's waveforms are %s: build the corpus with dtype=%s" % (pcm.dtype, pcm.dtype))
                pcm = pcm.to(dev, non_blocking=True)
            labels, tags, channels = _meta_ids(ds, meta, len(lens))
            corpus.append(pcm, lens, labels, tags, channels)
        if kind == "flac":
            flac.check(status.view())
            if status2.n:
                resample.check(status2.view())
        elif kind == "wav":
            wav.check(status.view())
        return corpus

    def sampler(self, batch_size, seed=688, ranges=None, ratio=None, shuffle=True, drop_last=None, Lcap=None,
                feat_len=750, hop=160, rank=None, world=None):
        """A stateful ``CorpusSampler`` over this corpus (see there)."""
        return CorpusSampler(self, batch_size, seed, ranges, ratio, shuffle, drop_last, Lcap, feat_len, hop, rank, world)


def _round_up_array(lens):
    return (np.asarray(lens, dtype=np.int64) + (ops.CORPUS_ALIGN - 1)) // ops.CORPUS_ALIGN * ops.CORPUS_ALIGN


def _meta_ids(ds, meta, B):
    """(labels, tags, channels | None) of a collated batch's meta ``[filename, tag, label[, channel ...]]``: integer
    tensors as the dataset.py classes give them, the protocol's strings mapped through ``ds.tag`` / ``ds.label`` for
    the raw classes (whose channel names have no class ids: no ``channels``)."""
    if len(meta) < 3:  # an unlabelled evaluation set: (waveform, filename)
        return torch.full((B,), -1, dtype=torch.int64), None, None
    tag, label = meta[1], meta[2]
    if torch.is_tensor(label):
        return label, tag, (meta[3] if len(meta) > 3 and torch.is_tensor(meta[3]) else None)
    from .dataset import LABEL
    label_map, tag_map = getattr(ds, "label", None) or LABEL, getattr(ds, "tag", None)  # (VCC2020Raw carries no tables)
    return (torch.tensor([label_map[v] for v in label], dtype=torch.int64),
            None if tag_map is None else torch.tensor([tag_map[v] for v in tag], dtype=torch.int64), None)


# ---------------------------------------------------------------------------------------------- device: the sampler
class CorpusSampler:
    """Ragged batches out of a ``DeviceCorpus`` without the host: ``for batch in sampler.epoch():`` yields
    ``DeviceBatch(pcm, labels, start, lengths, tags, channels, index)`` - the first four as Trainer.evaluate reads a
    batch and ``Trainer.step(b.pcm, b.labels, start=b.start, lengths=b.lengths)`` takes them.  Every field is a fresh
    device tensor of the batch's own; ``pcm`` is (B, Lcap) with zeros behind each row's length; ``start`` holds the
    crop offsets of dataset.py:69 (exclusive bound), drawn per utterance and generation.  Nothing in the loop
    synchronises.

    ``ranges`` (default the whole corpus) and ``ratio``: the flows, as ``Schedule`` documents.  ``shuffle=False`` walks
    the range in order and (``drop_last`` defaulting to ``shuffle``) keeps the short last batch - the dev / eval pass;
    while shuffling the short batch is dropped, so every training batch has one shape and one captured hipGraph
    serves them all.  ``rank`` / ``world`` default to the process group's.  ``Lcap``: a multiple of 8, at least the
    longest utterance of the ranges (default: that, rounded up to RAGGED_ROUND).  ``state_dict()`` carries generations
    and cursors; the permutations are functions of (seed, generation, flow) and are regenerated when needed."""

    def __init__(self, corpus, batch_size, seed=688, ranges=None, ratio=None, shuffle=True, drop_last=None, Lcap=None,
                 feat_len=750, hop=160, rank=None, world=None):
        if rank is None or world is None:
            from . import dist as air_dist
            rank = air_dist.rank() if rank is None else rank
            world = air_dist.world_size() if world is None else world
        n = len(corpus)
        if n < 1:
            raise ValueError("the corpus is empty")
        ranges = [(0, n)] if ranges is None else [(int(lo), int(hi)) for lo, hi in ranges]
        for lo, hi in ranges:
            if hi > n:
                raise ValueError("range (%d, %d) of a corpus of %d utterances" % (lo, hi, n))
        self.schedule = Schedule(ranges, batch_size, ratio, shuffle, drop_last, rank, world)
        self.Lcap = resolve_lcap(Lcap, corpus.host_lengths, self.schedule.ranges)
        self.corpus, self.seed = corpus, int(seed)
        self.feat_len, self.hop = int(feat_len), int(hop)
        if self.feat_len < 1 or self.hop < 1:
            raise ValueError("feat_len and hop are positive")
        self._perm = [None] * len(ranges)       # per flow: the device permutation and the generation it holds
        self._perm_gen = [None] * len(ranges)
        self._ws = None

    def __len__(self):
        return len(self.schedule)

    def state_dict(self):
        return self.schedule.state_dict()

    def load_state_dict(self, state):
        self.schedule.load_state_dict(state)

    def _permutation(self, flow, generation):
        if self._perm_gen[flow] != generation:
            lo, hi = self.schedule.ranges[flow]
            if self._perm[flow] is None:
                self._perm[flow] = torch.empty(hi - lo, dtype=torch.int64, device=self.corpus.device)
            if self._ws is None:
                # the sort's scratch is the sampler's own: growing the stream's shared workspace here would make a
                # trainer that replays a captured step capture it again (ops.workspace_generation)
                need = max(ops.corpus_permutation_ws_bytes(b - a) for a, b in self.schedule.ranges)
                self._ws = torch.empty(need, dtype=torch.uint8, device=self.corpus.device)
            # (stream order: the gathers that read the old permutation are enqueued ahead of this)
            ops.corpus_permutation(lo, hi - lo, self.seed, ops.corpus_stream(generation, flow), out=self._perm[flow],
                                   ws=self._ws)
            self._perm_gen[flow] = generation
        return self._perm[flow]

    def _batch(self, segs):
        c = self.corpus
        dsegs = []
        for flow, generation, first, count in segs:
            if count == 0:
                continue
            if self.schedule.shuffle:
                dsegs.append((self._permutation(flow, generation), first, count, generation))
            else:
                dsegs.append((None, self.schedule.ranges[flow][0] + first, count, generation))
        if not dsegs:
            return None
        return DeviceBatch(*ops.corpus_gather(c._samples, c._tables["offsets"], c._tables["lengths"], c._tables["labels"],
                                              c._tables["tags"], c._tables["index"],
                                              c._tables["channels"] if c.n_channels else None, c.n, dsegs, self.seed,
                                              self.feat_len, self.hop, self.Lcap))

    def epoch(self):
        """The batches of the next epoch (a generator; abandon it and ``epoch()`` starts the following epoch)."""
        self.schedule.begin_epoch()
        return self._rest()

    def resume(self):
        """The remaining batches of the epoch a loaded state stands in."""
        return self._rest()

    def _rest(self):
        while True:
            segs = self.schedule.next_step()
            if segs is None:
                return
            batch = self._batch(segs)
            if batch is not None:  # (shuffle=False, world > 1: a rank past the end of the range)
                yield batch
