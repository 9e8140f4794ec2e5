"""DiverGen copy-paste data path with the GPU compositor.

Host-side mirror of InstPool (DG/divergen/data/custom_build_copypaste_mapper.py:94-566) for the shipped
configuration (INST_POOL_FORMAT 'RGBA', INST_POOL_SAMPLE_TYPE 'cas_random', USE_COPY_METHOD 'syn_copy'): class-balanced sampling
of generated instances, size prior (Gaussian relative-area prior for LVIS classes with statistics, U(RANDOM_SCALE_MIN, MAX) of
the source size for the rest), random placement.  The four blend modes of INPUT.CP_METHOD (custom_cp_method.py:5-18):
  'basic', 'alpha', 'gaussian'   always built; per pixel, folded over the K pastes in one kernel
  'possion'                      Poisson blending (the reference's spelling), opt-in: this build's key INPUT.CP_POISSON (default false) admits
                                 it, without the key from_config refuses it.  One conjugate-gradient solve per paste on the device
                                 (csrc/poisson_blend.hip); it rewrites the image frame as the reference's poisson_edit does; composite()
                                 leaves the solver report unread (layers.copy_paste.check_poisson_report reads one)
Two halves:
  InstPool.prepare    numpy / PIL only, the reference's np.random call order (pinned on tests/golden/pool_draws.npz, draws of
                      the reference's own InstPool); runs in the DATALOADER.NUM_WORKERS loader processes and returns the K
                      patches packed into one flat buffer + descriptors (CPU tensors) + one blend mode per paste, drawn like
                      blend_image's `random.sample(cp_method, 1)[0]` from the pool's OWN random.Random (seeded by the loader's
                      _worker_init with the worker's seed, as D2's seed_all_rng seeds `random`; the process's global `random`
                      and the np.random stream are not touched)
  InstPool.composite  training process: upload + ONE call into libdgx (layers.copy_paste.copy_paste picks the entry point from the
                      modes: dgx_copy_paste, dgx_copy_paste_blend, or dgx_copy_paste_blend_ws with a 'possion' paste) for the
                      pixels -- image blend, mask occlusion updates, box recomputation and the occlusion filter of
                      `_copy_paste`, all pastes at once."""
import json
import os
import random
from collections import defaultdict

import numpy as np
import torch

from ..layers.copy_paste import BLEND_MODES, BLEND_MODES_ALL, PackedPastes, copy_paste
from ..structures import BitMasks, Boxes, DeviceResizeImage, DeviceResizePatch, Instances, PolygonCrossings


def check_cp_method(cp_method, allow_poisson=False):
    """INPUT.CP_METHOD -> list of mode names; every name must be a built blend mode (layers.copy_paste.BLEND_MODES), or 'possion'
    when allow_poisson (INPUT.CP_POISSON) says so."""
    names = [cp_method] if isinstance(cp_method, str) else list(cp_method)
    if not names:
        raise ValueError("INPUT.CP_METHOD is empty: name at least one of %s" % sorted(BLEND_MODES))
    for n in names:
        if n == "possion" and allow_poisson:
            continue
        if n == "possion":
            raise NotImplementedError("INPUT.CP_METHOD 'possion' is not built: the reference solves a sparse system over all H*W "
                                      "pixels per channel per paste (spsolve), which needs a GPU solver of its own")
        if n not in BLEND_MODES:
            raise NotImplementedError("INPUT.CP_METHOD '%s' is not a blend mode of this build (%s)" % (n, ", ".join(sorted(BLEND_MODES))))
    return names


def result_instances(out, with_source=True):
    """The result dict of layers.copy_paste.copy_paste / self_copy_paste (lazy_masks=True) -> the Instances of its image: gt_boxes,
    gt_classes, gt_masks (0/1 bytes: a bool view; the survivors' rows through the index) and, with_source, instance_source."""
    inst = Instances(tuple(int(v) for v in out["image"].shape[-2:]), gt_boxes=Boxes(out["boxes"]), gt_classes=out["labels"],
                     gt_masks=BitMasks(out["masks"].view(torch.bool), index=out["keep"]))
    if with_source:
        inst.instance_source = out["source"]
    return inst


def fill_device_masks(data, device):
    """INPUT.DEVICE_RASTER, training-process half: a sample whose instances carry PolygonCrossings gets its BitMasks here -- ONE
    dgx_polygons_to_bitmask launch into a fresh device tensor on the CURRENT stream (the loader's side stream), in front of
    dgx_remove_background and the compositor.  Any other sample is returned as it is."""
    inst = data.get("instances")
    if inst is None or not inst.has("gt_masks") or not isinstance(inst.gt_masks, PolygonCrossings):
        return data
    if torch.device(device).type != "cuda":
        raise RuntimeError("INPUT.DEVICE_RASTER needs the GPU kernel (dgx_polygons_to_bitmask); device is %s" % device)
    filled = Instances(inst.image_size)
    for name, value in inst.get_fields().items():
        filled.set(name, value.rasterize(device) if name == "gt_masks" else value)
    return dict(data, instances=filled)


# INPUT.DEVICE_RESIZE: a pool patch keeps its source crop (and is resized on the device) when the source has at most this many times the
# pixels of the resized patch; a larger source is resized by the worker, as without the key.  The factor bounds what the patch sources
# add to the sample blob: at most 4 x the bytes of `flat`, inside the ring slot's 8 MB for "the rest".
DEVICE_RESIZE_MAX_SRC_RATIO = 4


def materialize_resizes(data, device):
    """INPUT.DEVICE_RESIZE, training-process half: a sample whose image is a DeviceResizeImage gets its (3, ch, cw) uint8 tensor here,
    and the pool patches that were left to the device their bytes in `flat` -- ONE dgx_resize_bilinear_u8 launch on the CURRENT stream
    (the loader's side stream), in front of the mask fill, dgx_remove_background and the compositor.  From here on the sample is byte for
    byte what the key-off path carries.  Any other sample is returned as it is."""
    img = data.get("image")
    if not isinstance(img, DeviceResizeImage):
        return data
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("INPUT.DEVICE_RESIZE needs the GPU kernel (dgx_resize_bilinear_u8); device is %s" % device)
    from ..layers.resize_ops import resize_bilinear_u8
    from .resize_tables import assemble_jobs
    data = dict(data)
    pk = data.get("paste_pack")
    if img.pending is not None:                      # out of the blob: everything is on the device already, `flat` included
        p = img.pending
        src, jobs_host, tab_host, jobs_dev, tab_dev = p["src"], p["jobs_host"], p["tab_host"], p["jobs"], p["tab"]
        flat = pk["flat"] if pk is not None else None
    else:                                            # a sample that crossed unpacked (or never left this process)
        jobs, offs = [img.job], [0]
        flat = None
        if pk is not None:
            pk = data["paste_pack"] = dict(pk)
            for job, off in pk.pop("resize", ()):
                jobs.append(job)
                offs.append(off)
            if len(jobs) > 1:
                flat = pk["flat"] = pk["flat"].to(dev, non_blocking=True)
        src, jobs_host, tab_host = assemble_jobs(jobs, offs)
        src, jobs_dev, tab_dev = torch.from_numpy(src).to(dev, non_blocking=True), None, None
    out = torch.empty(img.shape, dtype=torch.uint8, device=dev)
    resize_bilinear_u8(src, jobs_host, tab_host, image=out, flat=flat, jobs_dev=jobs_dev, tab_dev=tab_dev)
    data["image"] = out
    return data


def largest_connected_component(mask):
    """Role of get_largest_connect_component (mapper.py:25-36, cv2 contours): keep the largest blob."""
    from scipy import ndimage
    lab, n = ndimage.label(mask)
    if n <= 1:
        return mask
    sizes = ndimage.sum(mask, lab, index=np.arange(1, n + 1))
    return (lab == (1 + int(np.argmax(sizes)))).astype(mask.dtype)


class InstPool:
    def __init__(self, pool_json, train_size, area_stats_json=None, max_samples=20, random_scale=False,
                 random_scale_min=0.1, random_scale_max=2.0, random_scale_min_size=5, use_largest_part=True,
                 scale_min=10, scale_max=0.5, shape_jitter=0.2, mask_threshold=128,
                 instance_filter_min=0.01, instance_filter_max=1.0, loader=None, cp_method=("basic",), allow_poisson=False):
        pool = json.load(open(pool_json)) if isinstance(pool_json, str) else pool_json
        self.per_cat_pool = defaultdict(list)
        self.dataset, self.data_to_cat = [], {}
        for cat, paths in pool.items():
            for p in paths:
                self.per_cat_pool[int(cat)].append(len(self.dataset))
                self.data_to_cat[p] = int(cat)          # pool json keys ARE the 0-based labels (mapper.py:143-152;
                                                        # written as `id - 1` by DG/filteration/clean_pool_if.py:173)
                self.dataset.append(p)
        self.cats = list(self.per_cat_pool.keys())
        self.HWms = json.load(open(area_stats_json)) if area_stats_json and os.path.exists(area_stats_json) else {}
        self.train_size, self.max_samples = train_size, max_samples
        self.random_scale, self.rs_min, self.rs_max, self.rs_min_size = random_scale, random_scale_min, random_scale_max, random_scale_min_size
        self.use_largest_part, self.scale_min, self.scale_max = use_largest_part, scale_min, scale_max
        self.shape_jitter, self.mask_threshold = shape_jitter, mask_threshold
        self.filter_min, self.filter_max = instance_filter_min, instance_filter_max
        self.loader = loader or self._pil_loader
        self.allow_poisson = bool(allow_poisson)
        self.cp_method = check_cp_method(cp_method, self.allow_poisson)
        self.device_resize = False        # INPUT.DEVICE_RESIZE (set by CopyPasteMapper): patches may leave load_rgba un-resized
        self.rng = random.Random()        # blend-mode draws only (seed: the loader's _worker_init); never the global `random`

    def seed(self, seed):
        """What D2's seed_all_rng does to `random` in a loader worker, done to the pool's own generator."""
        self.rng.seed(seed)

    @classmethod
    def from_config(cls, cfg):
        """The constructor call of CopyPasteMapper.from_config (mapper.py:726-745) for INST_POOL_FORMAT 'RGBA', including
        the category filter of InstPool.__init__ (:115-133: keep pool categories whose LVIS frequency is in INST_POOL_FREQ).
        INPUT.INST_POOL_SHARDS (this build's key) switches the per-sample decode to the shard store.  INPUT.CP_METHOD is checked
        here: unknown names raise NotImplementedError, and so does 'possion' unless INPUT.CP_POISSON (this build's key) is true."""
        with open(cfg.INPUT.INST_POOL_PATH) as f:
            pool = json.load(f)
        freq_path = cfg.MODEL.ROI_BOX_HEAD.CAT_FREQ_PATH
        if freq_path and os.path.exists(freq_path):
            with open(freq_path) as f:
                infos = json.load(f)
            select = {info["id"] - 1 for info in infos if info["frequency"] in cfg.INPUT.INST_POOL_FREQ}
            pool = {k: v for k, v in pool.items() if int(k) in select}
        loader = None
        if cfg.INPUT.get("INST_POOL_SHARDS", ""):
            from .pool_store import PoolStore
            loader = PoolStore(cfg.INPUT.INST_POOL_SHARDS).loader
        return cls(pool, cfg.INPUT.TRAIN_SIZE, area_stats_json=cfg.INPUT.MEAN_STD2_PATH,
                   max_samples=cfg.INPUT.INST_POOL_MAX_SAMPLES, random_scale=cfg.INPUT.RANDOM_SCALE,
                   random_scale_min=cfg.INPUT.RANDOM_SCALE_MIN, random_scale_max=cfg.INPUT.RANDOM_SCALE_MAX,
                   random_scale_min_size=cfg.INPUT.RANDOM_SCALE_MIN_SIZE, use_largest_part=cfg.USE_LARGEST_PART, loader=loader,
                   cp_method=cfg.INPUT.CP_METHOD, allow_poisson=bool(cfg.INPUT.get("CP_POISSON", False)))

    @staticmethod
    def _pil_loader(path):
        from PIL import Image
        mask_path = None
        if path.startswith("*"):
            path = path[1:]
        elif "|" in path:
            path, mask_path = path.split("|")[:2]
        rgba = np.array(Image.open(path).convert("RGBA"))
        if mask_path is not None:
            rgba[:, :, -1] = np.array(Image.open(mask_path))
        return rgba

    def sample_ids(self, nums):
        """_get_cls_balanced_random_samples (mapper.py:263-296): class first, then instance in class."""
        cats_pool = [self.per_cat_pool[c] for c in self.per_cat_pool if len(self.per_cat_pool[c]) > 0]
        ids = []
        if not cats_pool:
            return ids
        for _ in range(nums):
            cid = np.random.randint(0, len(cats_pool))
            ids.append(cats_pool[cid][np.random.randint(0, len(cats_pool[cid]))])
        return ids

    def load_rgba(self, key, image_hw):
        """_load_RGBA (mapper.py:359-456): returns (rgba (h,w,4) uint8, label) or None when rejected."""
        H, W = image_hw
        label = self.data_to_cat[key]
        try:
            rgba = self.loader(key)
        except Exception:
            return None
        if self.random_scale or str(label + 1) not in self.HWms:
            s = np.random.uniform(self.rs_min, self.rs_max)
            tw, th = int(rgba.shape[1] * s), int(rgba.shape[0] * s)
            if tw < self.rs_min_size or th < self.rs_min_size or tw >= W or th >= H:
                return None
        else:
            mean, std = self.HWms[str(label + 1)][:2]
            smin = self.scale_min / H if isinstance(self.scale_min, int) else self.scale_min
            smax = self.scale_max / H if isinstance(self.scale_max, int) else self.scale_max
            area = np.clip(mean + np.random.randn() * std, smin, smax)
            if not key.startswith("*"):
                seg = (rgba[..., 3:] > self.mask_threshold).astype("uint8")
                if self.use_largest_part:
                    seg = largest_connected_component(seg[..., 0])[..., None]
                ys, xs = np.where(seg[..., 0])
                frac = len(ys) / float(seg.shape[0] * seg.shape[1])
                if frac <= self.filter_min or frac >= self.filter_max:
                    return None
                y0, y1, x0, x1 = ys.min(), ys.max(), xs.min(), xs.max()
                if y1 <= y0 or x1 <= x0:
                    return None
                rgba[:, :, 3:] *= seg
                rgba = rgba[y0:y1 + 1, x0:x1 + 1]
            scale = area ** 2 * H * W
            ratio = rgba.shape[1] / rgba.shape[0] * np.random.uniform(1 - self.shape_jitter, 1 + self.shape_jitter)
            tw = np.sqrt(ratio * scale)
            th = tw / ratio
            tw, th = int(tw), int(th)
            if tw < 5 or tw >= W or th < 5 or th >= H:
                return None
        if self.device_resize and rgba.shape[0] * rgba.shape[1] <= DEVICE_RESIZE_MAX_SRC_RATIO * th * tw:
            rgba = DeviceResizePatch(rgba, th, tw)                                          # INPUT.DEVICE_RESIZE: resized (and flipped) on the device
        else:
            rgba = self._resize(rgba, tw, th)
        if np.random.rand() < 0.5:                                                          # RandomFlip(horizontal)
            if isinstance(rgba, DeviceResizePatch):
                rgba.flip = True                                                            # its job mirrors the resized patch
            else:
                rgba = np.ascontiguousarray(rgba[:, ::-1])
        return rgba, label

    @staticmethod
    def _resize(rgba, tw, th):
        """cv2.resize(img_RGBA, (target_W, target_H)) role (mapper.py:446); cv2 is not in this image, PIL bilinear is."""
        from PIL import Image
        return np.array(Image.fromarray(np.ascontiguousarray(rgba), "RGBA").resize((tw, th), Image.BILINEAR))

    @staticmethod
    def random_start_xy(rgba, train_hw):
        """random_start_xy (mapper.py:45-57): offsets so that the patch centre stays inside the canvas."""
        h, w = rgba.shape[:2]
        x_mid, y_mid = (0 + w) / 2.0, (0 + h) / 2.0
        H, W = train_hw
        return np.random.randint(-x_mid, W - x_mid), np.random.randint(-y_mid, H - y_mid)

    def draw(self, image_hw):
        """The random part of get_mix_result('cas_random') + _cat_a_new_image (mapper.py:213-261, :488-496) for one image of size
        image_hw, in the reference's np.random order: the number of samples, the (class, instance) pairs, then EVERY _load_RGBA
        (size prior / scale, jitter, flip), and only then the placement of the instances that survived
        (`datas = [self._load_RGBA(...) ...]` completes before `datas = [random_start_xy(...) ...]` starts).
        Returns (pastes [(rgba (h,w,4) uint8, x0, y0, label)], names).  Pure numpy / PIL: this is what a loader worker runs."""
        H, W = image_hw
        num = np.random.randint(0, self.max_samples)
        keys = [self.dataset[i] for i in self.sample_ids(num)]
        loaded = []
        for key in keys:
            r = self.load_rgba(key, (H, W))
            if r is not None:
                loaded.append((r[0], int(r[1]), str(key)))
        pastes, names = [], []
        for rgba, label, key in loaded:
            x0, y0 = self.random_start_xy(rgba, (H, W))
            pastes.append((rgba, int(x0), int(y0), label))
            names.append(key)
        return pastes, names

    def draw_modes(self, K):
        """The blend mode of each of K surviving pastes, in paste order: blend_image's `random.sample(cp_method, 1)[0]`
        (custom_cp_method.py:6, one call per _copy_paste, even for a one-element list) on the pool's own generator.
        The sequence equals blend_image's own draws from the same seed.  In the reference, `random` also feeds the
        albumentations Compose that every loaded patch passes through first (mapper.py:496, `cumstom_augmentations`, empty
        unless INPUT.COLOR_AUG): whether that draws from the global `random`, and how often, depends on the albumentations
        version, which the reference does not pin.  Those draws are not replayed here; the per-paste distribution is the same."""
        return np.array([BLEND_MODES_ALL[self.rng.sample(self.cp_method, 1)[0]] for _ in range(K)], dtype=np.uint8)

    def prepare(self, data):
        """Loader-worker half of get_mix_result: draw + decode + clean + resize + flip + place + pack.  Adds to the mapped sample
        `paste_pack` = dict(flat uint8, desc int32 (K,5), labels int64 (K), K) -- CPU tensors, the compositor's input form -- plus
        `modes`, the K blend-mode bytes as a numpy uint8 array (host data, never uploaded; data/build.py hands it over outside the
        blob, and only when some paste is not 'basic') -- and `paste_labels` / `paste_filename_list` (BSGAL's selection reads these).  No device, no libdgx."""
        from ..layers.copy_paste import pack_pastes_host
        H, W = data["image"].shape[-2:]
        pastes, names = self.draw((H, W))
        flat, desc, labels = pack_pastes_host(pastes)
        data = dict(data)
        data["paste_pack"] = {"flat": flat, "desc": desc, "labels": labels, "modes": self.draw_modes(len(pastes)),
                              "K": len(pastes)}
        # INPUT.DEVICE_RESIZE: one interleaved RGBA job per patch left to the device, its destination the patch's range of `flat`
        resize = [(p[0].job(), int(d[0])) for p, d in zip(pastes, desc.tolist()) if isinstance(p[0], DeviceResizePatch)]
        if resize:
            data["paste_pack"]["resize"] = resize
        data["paste_labels"], data["paste_filename_list"] = [p[3] for p in pastes], names
        return data

    @staticmethod
    def composite(data, device):
        """Training-process half: the prepared sample's tensors go to `device` (asynchronously when they are pinned) and ONE
        libdgx call (copy_paste) on the CURRENT stream blends all K patches, updates masks / boxes and drops covered objects.  The
        caller chooses the stream (data/build.py: a side stream, one batch ahead of the training stream)."""
        data = materialize_resizes(data, device)     # INPUT.DEVICE_RESIZE: the image and the device-resized patches, before they are read
        data = fill_device_masks(data, device)       # INPUT.DEVICE_RASTER: the ground-truth masks are filled here, before they are read
        pk = data["paste_pack"]
        inst = data["instances"]
        H, W = data["image"].shape[-2:]
        up = lambda t: t.to(device, non_blocking=True)     # noqa: E731
        image, gm = up(data["image"]), up(inst.gt_masks.tensor.view(torch.uint8))
        gb, gc = up(inst.gt_boxes.tensor), up(inst.gt_classes)
        # modes stay on the host, and so do the descriptors wherever they already are there (the loader's `desc_host`, a pack not yet uploaded)
        desc_host = pk.get("desc_host", None if pk["desc"].is_cuda else pk["desc"].numpy())
        packed = PackedPastes(up(pk["flat"]), up(pk["desc"]), up(pk["labels"]), int(pk["K"]), pk.get("modes"), desc_host)
        out = copy_paste(image, gm, gb, gc, packed, lazy_masks=True, allow_poisson=True)      # the pool refused 'possion' where it is off
        data = {k: v for k, v in data.items() if k != "paste_pack"}
        data["image"], data["instances"], data["height"], data["width"] = out["image"], result_instances(out), H, W
        data["_uploaded"] = (image, gm, gb, gc)      # the un-pasted sample on the device (BSGAL keeps it; copy_paste wrote a clone)
        return data

    def __call__(self, data):
        """get_mix_result('cas_random') (mapper.py:213-261) on one mapped sample dict, both halves in this process."""
        dev = data["image"].device if data["image"].is_cuda else torch.device("cuda")
        data = self.composite(self.prepare(data), dev)
        data.pop("_uploaded", None)
        return data
