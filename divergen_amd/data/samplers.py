"""Rank-sharded index streams for the training / evaluation loaders.

The contract is the reference's (D2/data/samplers/distributed_sampler.py:15-70 TrainingSampler, :129-243
RepeatFactorTrainingSampler, :245-278 InferenceSampler): every rank builds the SAME seeded stream and keeps every
world_size-th element starting at its rank.  What has to match the reference bit for bit is the order of the draws on the one
CPU generator -- `rand(n)` for the fractional repeats, then `randperm(len(epoch))` -- so that a run here visits the images in
the reference's order for the same seed (tests/golden/samplers.npz holds streams of the reference's own classes).
"""
import math

import torch

from ..utils import comm


def _rank_share(stream, rank, world):
    """Every world-th element of an endless stream, starting at `rank`."""
    for k, idx in enumerate(stream):
        if k % world == rank:
            yield idx


class _SeededStream:
    """Seed / rank / world bookkeeping shared by the two training samplers; subclasses provide `epoch(generator)` -> 1-D int64
    tensor of dataset indices for one pass."""

    def __init__(self, shuffle, seed, rank, world_size):
        self.shuffle = bool(shuffle)
        self.seed = int(comm.shared_random_seed() if seed is None else seed)
        self.rank = comm.get_rank() if rank is None else int(rank)
        self.world = comm.get_world_size() if world_size is None else int(world_size)

    def epoch(self, generator):
        raise NotImplementedError

    def stream(self):
        gen = torch.Generator().manual_seed(self.seed)
        while True:
            ids = self.epoch(gen)
            if self.shuffle:
                ids = ids[torch.randperm(ids.numel(), generator=gen)]
            yield from ids.tolist()

    def __iter__(self):
        return _rank_share(self.stream(), self.rank, self.world)


class TrainingSampler(_SeededStream):
    """Endless passes over range(size), each pass a fresh permutation of the shared generator (or 0..size-1 when not shuffling)."""

    def __init__(self, size, shuffle=True, seed=None, rank=None, world_size=None):
        if size <= 0:
            raise ValueError("TrainingSampler needs a non-empty dataset")
        super().__init__(shuffle, seed, rank, world_size)
        self.size = int(size)

    def epoch(self, generator):
        return torch.arange(self.size)


class RepeatFactorTrainingSampler(_SeededStream):
    """LVIS repeat-factor sampling (Gupta et al. 2019, sec. 4.1): image i appears floor(r_i) times per pass plus once more
    with probability frac(r_i)."""

    def __init__(self, repeat_factors, *, shuffle=True, seed=None, rank=None, world_size=None):
        super().__init__(shuffle, seed, rank, world_size)
        rf = torch.as_tensor(repeat_factors, dtype=torch.float32)
        self.whole = torch.trunc(rf)
        self.frac = rf - self.whole

    @staticmethod
    def repeat_factors_from_category_frequency(dataset_dicts, repeat_thresh):
        """r(image) = max over its categories c of max(1, sqrt(t / f(c))), f(c) = share of images that contain c; images
        without annotations get 1."""
        per_image = [{a["category_id"] for a in d["annotations"]} for d in dataset_dicts]
        images_with = {}
        for cats in per_image:
            for cid in cats:
                images_with[cid] = images_with.get(cid, 0) + 1
        n = len(dataset_dicts)
        cat_rep = {cid: max(1.0, math.sqrt(repeat_thresh / (cnt / n))) for cid, cnt in images_with.items()}
        return torch.tensor([max((cat_rep[cid] for cid in cats), default=1.0) for cats in per_image], dtype=torch.float32)

    def epoch(self, generator):
        extra = torch.rand(self.frac.numel(), generator=generator) < self.frac
        counts = (self.whole + extra.to(self.whole.dtype)).to(torch.int64)
        return torch.repeat_interleave(torch.arange(counts.numel()), counts)


def repeat_factors_from_tag_frequency(dataset_dicts, repeat_thresh):
    """DG/divergen/data/custom_dataset_dataloader.py:481-504: the repeat factors of an image-labelled source, from the frequency of
    its `pos_category_ids` instead of box annotations; an image without labels gets 1."""
    freq = {}
    for d in dataset_dicts:
        for cid in d["pos_category_ids"]:
            freq[cid] = freq.get(cid, 0) + 1
    n = len(dataset_dicts)
    cat_rep = {cid: max(1.0, math.sqrt(repeat_thresh / (cnt / n))) for cid, cnt in freq.items()}
    return torch.tensor([max({cat_rep[cid] for cid in d["pos_category_ids"]}, default=1.0) for d in dataset_dicts], dtype=torch.float32)


class MultiDatasetSampler:
    """DG/divergen/data/custom_dataset_dataloader.py:368-438: indices into the CONCATENATION of several sources (`dataset_source` on
    every dict, sources back to back), drawn with replacement.  Image i of source s weighs max(sizes) / size_s * ratio_s / sum(ratio)
    times its repeat factor; with USE_RFS[s] that is the category-frequency factor of a 'box' source and the tag-frequency factor of
    any other, rescaled to sum to size_s.  One `torch.multinomial(weights, N, replacement=True)` per pass on the shared seeded
    generator, every world_size-th index starting at the rank."""

    def __init__(self, dataset_dicts, dataset_ratio, use_rfs, dataset_ann, repeat_threshold=0.001, seed=None, rank=None, world_size=None):
        n_src = len(dataset_ratio)
        sizes = [0] * n_src
        for d in dataset_dicts:
            sizes[d["dataset_source"]] += 1
        if min(sizes) == 0:
            raise ValueError("MultiDatasetSampler: dataset sizes %s for %d DATALOADER.DATASET_RATIO entries" % (sizes, n_src))
        self.sizes = sizes
        self.seed = int(comm.shared_random_seed() if seed is None else seed)
        self.rank = comm.get_rank() if rank is None else int(rank)
        self.world = comm.get_world_size() if world_size is None else int(world_size)
        self.dataset_ids = torch.tensor([d["dataset_source"] for d in dataset_dicts], dtype=torch.long)
        weight = torch.cat([torch.ones(s) * max(sizes) / s * r / sum(dataset_ratio) for r, s in zip(dataset_ratio, sizes)])
        factors, st = [], 0
        for i, s in enumerate(sizes):
            if use_rfs[i]:
                fn = RepeatFactorTrainingSampler.repeat_factors_from_category_frequency if dataset_ann[i] == "box" \
                    else repeat_factors_from_tag_frequency
                f = fn(dataset_dicts[st:st + s], repeat_threshold)
                f = f * (s / f.sum())
            else:
                f = torch.ones(s)
            factors.append(f)
            st += s
        self.weights = weight * torch.cat(factors)

    def stream(self):
        gen = torch.Generator().manual_seed(self.seed)
        while True:
            yield from torch.multinomial(self.weights, len(self.weights), generator=gen, replacement=True).tolist()

    def __iter__(self):
        return _rank_share(self.stream(), self.rank, self.world)


class GroupedBatchSampler:
    """The batches of MDAspectRatioGroupedDataset / DIFFMDAspectRatioGroupedDataset (custom_dataset_dataloader.py:441-478) formed
    BEFORE the samples are mapped: a batch sampler over the rank's index stream.  Index i goes to bucket
    `dataset_source * 2 + (0 if width > height else 1)` of its dataset dict; a bucket is emitted, in arrival order, when it holds
    the batch size -- `batch_sizes[source]` (USE_DIFF_BS_SIZE: DATALOADER.DATASET_BS) or the one per-GPU size.  Same composition
    and order as grouping the mapped samples, and a batch never mixes sources, so it never mixes annotation types."""

    def __init__(self, sampler, dataset_dicts, batch_sizes):
        self.sampler = sampler
        self.bucket_of = [d["dataset_source"] * 2 + (0 if d["width"] > d["height"] else 1) for d in dataset_dicts]
        self.batch_sizes = [int(b) for b in batch_sizes]
        n_src = max(d["dataset_source"] for d in dataset_dicts) + 1
        if len(self.batch_sizes) == 1:
            self.batch_sizes = self.batch_sizes * n_src
        if len(self.batch_sizes) < n_src or min(self.batch_sizes) < 1:
            raise ValueError("GroupedBatchSampler: batch sizes %s for %d sources" % (batch_sizes, n_src))

    def __iter__(self):
        buckets = {}
        for i in self.sampler:
            b = self.bucket_of[i]
            bucket = buckets.setdefault(b, [])
            bucket.append(i)
            if len(bucket) == self.batch_sizes[b // 2]:
                yield bucket[:]
                del bucket[:]


class InferenceSampler:
    """Contiguous shards of range(size), sizes differing by at most one (the first size % world ranks take the extra)."""

    def __init__(self, size, rank=None, world_size=None):
        rank = comm.get_rank() if rank is None else int(rank)
        world = comm.get_world_size() if world_size is None else int(world_size)
        self.shard = self._get_local_indices(int(size), world, rank)

    @staticmethod
    def _get_local_indices(total_size, world_size, rank):
        base, extra = divmod(total_size, world_size)
        start = rank * base + min(rank, extra)
        return range(start, start + base + (1 if rank < extra else 0))

    def __iter__(self):
        return iter(self.shard)

    def __len__(self):
        return len(self.shard)
