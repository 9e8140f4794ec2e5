"""The real training data path: dataset json -> dataset dicts -> DatasetMapper (+ EfficientDetResizeCrop, RandomFlip) ->
instance copy-paste from the pool (GPU compositor) -> batches with the model's input contract.

Host-side mirror (CPU workers, numpy / PIL as in the reference) of
  DG/divergen/data/datasets/lvis_v1.py:27-119            custom_load_lvis_json  (here without lvis-api: plain json)
  D2/data/datasets/builtin.py + lvis.py                  the lvis_v1_* split table under $DETECTRON2_DATASETS
  D2/data/build.py:get_detection_dataset_dicts           empty-annotation filter
  DG/divergen/data/custom_build_augmentation.py:13-46    build_custom_augmentation
  DG/divergen/data/transforms/custom_augmentation_impl.py:24-72, custom_transform.py:27-91   EfficientDetResizeCrop
  D2/data/transforms/augmentation_impl.py RandomFlip, fvcore HFlipTransform
  DG/divergen/data/dataset_mapper.py:127-256             DatasetMapper.__call__ (training branch, bitmask / polygon masks)
  D2/data/detection_utils.py                             read_image, transform_instance_annotations, annotations_to_instances,
                                                         filter_empty_instances
  DG/divergen/data/custom_build_copypaste_mapper.py:856-958   CopyPasteMapper.__call__ for USE_COPY_METHOD 'syn_copy'
  DG/train_net.py:164-239                                mapper / sampler / loader assembly
Random draws use np.random in the reference's order (scale factor, offset_y, offset_x, flip), so a seeded worker walks the
same augmentation stream.  Polygon rasterisation restates pycocotools' rleFrPoly (maskApi.c; pycocotools is not vendored
by the reference and absent here: PARITY UNPINNED by reference vectors, pinned by known answers in tests/test_host_data.py).
"""
import copy
import gc
import json
import logging
import os

import numpy as np
import torch

from ..structures import BitMasks, Boxes, DeviceResizeImage, Instances, PolygonCrossings
from ..utils import comm
from .samplers import RepeatFactorTrainingSampler, TrainingSampler

logger = logging.getLogger("divergen_amd")

# (image root, json) relative to $DETECTRON2_DATASETS: D2/data/datasets/builtin.py:_PREDEFINED_SPLITS_LVIS["lvis_v1"] and
# DG/divergen/data/datasets/lvis_v1.py:_CUSTOM_SPLITS_LVIS
SPLITS = {
    "lvis_v1_train": ("coco/", "lvis/lvis_v1_train.json"),
    "lvis_v1_val": ("coco/", "lvis/lvis_v1_val.json"),
    "lvis_v1_test_dev": ("coco/", "lvis/lvis_v1_image_info_test_dev.json"),
    "lvis_v1_test_challenge": ("coco/", "lvis/lvis_v1_image_info_test_challenge.json"),
    "lvis_v1_dev_val": ("coco/", "lvis/lvis_v1_dev_val.json"),
    "lvis_v1_mini_train": ("coco/", "lvis/lvis_v1_mini_train.json"),
    "lvis_v1_train_norare": ("coco/", "lvis/lvis_v1_train_norare.json"),
}
_REGISTERED = {}


def register_lvis_instances(name, json_file, image_root):
    _REGISTERED[name] = (json_file, image_root)


def dataset_files(name):
    if name in _REGISTERED:
        return _REGISTERED[name]
    if name not in SPLITS:
        raise KeyError("Dataset '{}' is not registered! Available: {}".format(name, sorted(list(SPLITS) + list(_REGISTERED))))
    root = os.getenv("DETECTRON2_DATASETS", "datasets")
    image_root, json_file = SPLITS[name]
    return os.path.join(root, json_file), os.path.join(root, image_root)


def load_lvis_json(json_file, image_root):
    """custom_load_lvis_json (lvis_v1.py:27-119): records with file_name / height / width / image_id /
    neg_category_ids (0-based) / not_exhaustive_category_ids / annotations (bbox XYWH, 0-based category_id, polygons)."""
    if not os.path.isfile(json_file):
        raise FileNotFoundError("LVIS annotation file {} not found (DETECTRON2_DATASETS={})".format(
            json_file, os.getenv("DETECTRON2_DATASETS", "datasets")))
    with open(json_file) as f:
        ds = json.load(f)
    cats = sorted(ds["categories"], key=lambda x: x["id"])
    catid2contid = {x["id"]: i for i, x in enumerate(cats)}
    if len(cats) == 1203:
        assert all(catid2contid[x["id"]] == x["id"] - 1 for x in cats)
    img_ann = {}
    for ann in ds.get("annotations", []):
        img_ann.setdefault(ann["image_id"], []).append(ann)
    ann_ids = [a["id"] for v in img_ann.values() for a in v]
    assert len(set(ann_ids)) == len(ann_ids), "Annotation ids in '{}' are not unique".format(json_file)
    out = []
    for img in sorted(ds["images"], key=lambda x: x["id"]):
        rec = {}
        if "file_name" in img:
            fn = img["file_name"]
            if fn.startswith("COCO"):
                fn = fn[-16:]
            rec["file_name"] = os.path.join(image_root, fn)
        elif "coco_url" in img:
            rec["file_name"] = os.path.join(image_root, img["coco_url"][30:])     # .../train2017/000000391895.jpg
        for k in ("height", "width"):
            if k in img:
                rec[k] = img[k]
        rec["not_exhaustive_category_ids"] = img.get("not_exhaustive_category_ids", [])
        rec["neg_category_ids"] = [catid2contid[x] for x in img.get("neg_category_ids", [])]
        if "pos_category_ids" in img:
            rec["pos_category_ids"] = [catid2contid[x] for x in img["pos_category_ids"]]
        if "captions" in img:               # lvis_v1.py:91-92: the captions of a caption-supervised image ride on the record
            rec["captions"] = img["captions"]
        image_id = rec["image_id"] = img["id"]
        objs = []
        for anno in img_ann.get(image_id, []):
            assert anno["image_id"] == image_id
            if anno.get("iscrowd", 0) > 0:
                continue
            obj = {"bbox": anno["bbox"], "bbox_mode": "XYWH_ABS", "category_id": catid2contid[anno["category_id"]]}
            if "segmentation" in anno:
                segm = anno["segmentation"]
                assert len(segm) > 0
                obj["segmentation"] = segm
            objs.append(obj)
        rec["annotations"] = objs
        out.append(rec)
    logger.info("Loaded {} images in the LVIS v1 format from {}".format(len(out), json_file))
    return out


def get_detection_dataset_dicts(names, filter_empty=True):
    """D2/data/build.py:get_detection_dataset_dicts for instance datasets: concatenate, drop images without annotations."""
    if isinstance(names, str):
        names = [names]
    dicts = []
    for n in names:
        d = load_lvis_json(*dataset_files(n))
        assert len(d), "Dataset '{}' is empty!".format(n)
        dicts.extend(d)
    if filter_empty:
        before = len(dicts)
        dicts = [d for d in dicts if any(a.get("iscrowd", 0) == 0 for a in d["annotations"])]
        logger.info("Removed {} images with no usable annotations. {} images left.".format(before - len(dicts), len(dicts)))
    return dicts


def get_detection_dataset_dicts_with_source(names, filter_empty=True, dataset_ann=None):
    """DG/divergen/data/custom_dataset_dataloader.py:333-365: the sources concatenated in the order of DATASETS.TRAIN, every dict
    tagged with `dataset_source` = its source's position.  The reference filters images without box annotations over the whole
    concatenation whenever the first dict has `annotations` -- which would silently delete every image-labelled source -- so
    DATALOADER.FILTER_EMPTY_ANNOTATIONS is refused by name when a source is not 'box'."""
    if isinstance(names, str):
        names = [names]
    assert len(names)
    if dataset_ann is not None:
        from ..config.image_labels import check_filter_empty
        check_filter_empty(filter_empty, list(dataset_ann)[:len(names)])
    dicts = []
    for source, n in enumerate(names):
        d = load_lvis_json(*dataset_files(n))
        assert len(d), "Dataset '{}' is empty!".format(n)
        for rec in d:
            rec["dataset_source"] = source
        dicts.extend(d)
    if filter_empty:
        before = len(dicts)
        dicts = [d for d in dicts if any(a.get("iscrowd", 0) == 0 for a in d["annotations"])]
        logger.info("Removed {} images with no usable annotations. {} images left.".format(before - len(dicts), len(dicts)))
    return dicts


# ----------------------------------------------------------------------------------------------- transforms
class EfficientDetResizeCropTransform:
    """custom_transform.py:27-91 (uint8 images through PIL, coordinates scaled then shifted)."""

    def __init__(self, scaled_h, scaled_w, offset_y, offset_x, img_scale, target_size):
        self.scaled_h, self.scaled_w, self.offset_y, self.offset_x = scaled_h, scaled_w, offset_y, offset_x
        self.img_scale, self.target_size = img_scale, target_size

    def apply_image(self, img, nearest=False):
        from PIL import Image
        assert img.dtype == np.uint8
        pil = Image.fromarray(img).resize((self.scaled_w, self.scaled_h), Image.NEAREST if nearest else Image.BILINEAR)
        ret = np.asarray(pil)
        right = min(self.scaled_w, self.offset_x + self.target_size[1])
        lower = min(self.scaled_h, self.offset_y + self.target_size[0])
        return ret[self.offset_y:lower, self.offset_x:right]

    def apply_coords(self, coords):
        coords[:, 0] = coords[:, 0] * self.img_scale
        coords[:, 1] = coords[:, 1] * self.img_scale
        coords[:, 0] -= self.offset_x
        coords[:, 1] -= self.offset_y
        return coords


class HFlipTransform:
    def __init__(self, width):
        self.width = width

    def apply_image(self, img, nearest=False):
        return np.flip(img, axis=1)

    def apply_coords(self, coords):
        coords[:, 0] = self.width - coords[:, 0]
        return coords


class NoOpTransform:
    def apply_image(self, img, nearest=False):
        return img

    def apply_coords(self, coords):
        return coords


class EfficientDetResizeCrop:
    """custom_augmentation_impl.py:24-72: random scale of the target square, then a random crop offset."""

    def __init__(self, size, scale):
        self.target_size = (size, size) if size > 0 else None
        self.scale = scale

    def get_transform(self, img):
        scale_factor = np.random.uniform(*self.scale)
        width, height = img.shape[1], img.shape[0]
        if self.target_size is not None:
            img_scale = min(scale_factor * self.target_size[0] / height, scale_factor * self.target_size[1] / width)
        else:
            img_scale = scale_factor
        scaled_h = max(1, int(height * img_scale))
        scaled_w = max(1, int(width * img_scale))
        if self.target_size is not None:
            offset_y, offset_x, target_size = scaled_h - self.target_size[0], scaled_w - self.target_size[1], self.target_size
        else:
            offset_y, offset_x, target_size = 0, 0, (scaled_h, scaled_w)
        offset_y = int(max(0.0, float(offset_y)) * np.random.uniform(0, 1))
        offset_x = int(max(0.0, float(offset_x)) * np.random.uniform(0, 1))
        return EfficientDetResizeCropTransform(scaled_h, scaled_w, offset_y, offset_x, img_scale, target_size)


class ResizeTransform:
    """fvcore / D2 ResizeTransform: PIL bilinear for uint8 images, coordinates scaled per axis."""

    def __init__(self, h, w, new_h, new_w):
        self.h, self.w, self.new_h, self.new_w = h, w, new_h, new_w

    def apply_image(self, img, nearest=False):
        from PIL import Image
        assert img.shape[:2] == (self.h, self.w)
        return np.asarray(Image.fromarray(img).resize((self.new_w, self.new_h), Image.NEAREST if nearest else Image.BILINEAR))

    def apply_coords(self, coords):
        coords[:, 0] = coords[:, 0] * (self.new_w * 1.0 / self.w)
        coords[:, 1] = coords[:, 1] * (self.new_h * 1.0 / self.h)
        return coords


class ResizeShortestEdge:
    """D2/data/transforms/augmentation_impl.py ResizeShortestEdge: shortest edge to `short` (one of a list, np.random.choice),
    longest edge capped at max_size; the evaluation input of D2's default DatasetMapper (INPUT.MIN_SIZE_TEST / MAX_SIZE_TEST)."""

    def __init__(self, short, max_size, sample_style="choice"):
        self.short = (short, short) if isinstance(short, int) else tuple(short)
        self.max_size, self.is_range = max_size, sample_style == "range"

    def get_transform(self, img):
        h, w = img.shape[:2]
        size = np.random.randint(self.short[0], self.short[1] + 1) if self.is_range else np.random.choice(self.short)
        if size == 0:
            return NoOpTransform()
        scale = size * 1.0 / min(h, w)
        newh, neww = (size, scale * w) if h < w else (scale * h, size)
        if max(newh, neww) > self.max_size:
            scale = self.max_size * 1.0 / max(newh, neww)
            newh, neww = newh * scale, neww * scale
        return ResizeTransform(h, w, int(newh + 0.5), int(neww + 0.5))


class RandomFlip:
    """D2 RandomFlip(prob=0.5, horizontal=True): one np.random.uniform draw."""

    def __init__(self, prob=0.5):
        self.prob = prob

    def get_transform(self, img):
        return HFlipTransform(img.shape[1]) if np.random.uniform() < self.prob else NoOpTransform()


def build_custom_augmentation(cfg, is_train):
    """custom_build_augmentation.py:13-46 for INPUT.CUSTOM_AUG == 'EfficientDetResizeCrop' (the shipped configs)."""
    if cfg.INPUT.CUSTOM_AUG != "EfficientDetResizeCrop":
        raise NotImplementedError("INPUT.CUSTOM_AUG '{}': only EfficientDetResizeCrop (the shipped configs) is built".format(cfg.INPUT.CUSTOM_AUG))
    if is_train:
        aug = [EfficientDetResizeCrop(cfg.INPUT.TRAIN_SIZE, tuple(cfg.INPUT.SCALE_RANGE)), RandomFlip()]
    else:
        aug = [EfficientDetResizeCrop(cfg.INPUT.TEST_SIZE, (1, 1))]
    return aug


# ----------------------------------------------------------------------------------------------- polygons -> bitmask
def polygon_crossings(xy, h, w):
    """pycocotools maskApi.c rleFrPoly up to its sort: the column-major flat positions at which the fill toggles, for one polygon
    given as a flat [x0, y0, x1, y1, ...] list.  Restated from the published C source -- 5x upsampled integer polygon, all
    boundary points by the longer-axis walk, the points where the boundary crosses a pixel-column centre -- as numpy array
    arithmetic (a loader worker rasterises ~12 polygons per image; the per-point Python loop of round 1-5 cost 5 ms each)."""
    k = len(xy) // 2
    scale = 5.0
    pts = np.asarray(xy, dtype=np.float64).reshape(k, 2)
    x = (scale * pts[:, 0] + 0.5).astype(np.int64)              # C (int) cast: truncation toward zero, as astype does
    y = (scale * pts[:, 1] + 0.5).astype(np.int64)
    x, y = np.append(x, x[0]), np.append(y, y[0])
    us, vs = [], []
    for j in range(k):
        xs, xe, ys, ye = int(x[j]), int(x[j + 1]), int(y[j]), int(y[j + 1])
        dx, dy = abs(xe - xs), abs(ys - ye)
        flip = (dx >= dy and xs > xe) or (dx < dy and ys > ye)
        if flip:
            xs, xe, ys, ye = xe, xs, ye, ys
        if dx >= dy:
            s = 0.0 if dx == 0 else (ye - ys) / dx
            t = np.arange(dx, -1, -1) if flip else np.arange(dx + 1)
            us.append(t + xs)
            vs.append((ys + s * t + 0.5).astype(np.int64))
        else:
            s = 0.0 if dy == 0 else (xe - xs) / dy
            t = np.arange(dy, -1, -1) if flip else np.arange(dy + 1)
            vs.append(t + ys)
            us.append((xs + s * t + 0.5).astype(np.int64))
    u, v = np.concatenate(us), np.concatenate(vs)
    # points along the y-boundary, downsampled
    u1, u0, v1, v0 = u[1:], u[:-1], v[1:], v[:-1]
    sel = u1 != u0
    u1, u0, v1, v0 = u1[sel], u0[sel], v1[sel], v0[sel]
    xd = (np.where(u1 < u0, u1, u1 - 1).astype(np.float64) + 0.5) / scale - 0.5
    ok = (np.floor(xd) == xd) & (xd >= 0) & (xd <= w - 1)
    yd = (np.where(v1 < v0, v1, v0).astype(np.float64) + 0.5) / scale - 0.5
    yd = np.ceil(np.clip(yd, 0.0, float(h)))
    return xd[ok].astype(np.int64) * h + yd[ok].astype(np.int64)


def polygon_to_rle_counts(xy, h, w):
    """The run lengths rleFrPoly returns (column-major, first run = zeros): sorted crossings -> differences -> zero-length
    runs merged into their neighbours (the first run may be zero).  Kept for the known-answer tests; the mapper fills masks
    from the crossings directly (polygons_to_bitmask)."""
    a = sorted(int(p) for p in polygon_crossings(xy, h, w))
    a.append(h * w)
    p = 0
    for j in range(len(a)):
        t = a[j]
        a[j] -= p
        p = t
    b = []
    j = 0
    if a:
        b.append(a[0])
        j = 1
    while j < len(a):
        if a[j] > 0:
            b.append(a[j])
            j += 1
        else:
            j += 1
            if j < len(a):
                b[-1] += a[j]
                j += 1
    return b


def polygons_to_bitmask(polygons, h, w, out=None):
    """D2/structures/masks.py:polygons_to_bitmask: union (rleMerge) of the polygons of one instance, decoded (h, w) bool
    (row-major; written into `out` when given).  Decoding the run lengths of rleFrPoly = the parity of the number of crossings
    at or before each column-major position (a zero-length run is two toggles at one position); only the columns between the
    first and the last crossing are computed, and transposed into the row-major mask."""
    m = np.zeros((h, w), dtype=bool) if out is None else out
    for poly in polygons:
        pos = polygon_crossings([float(c) for c in poly], h, w)
        pos = pos[pos < h * w]
        if pos.size == 0:
            continue
        c0, c1 = int(pos.min()) // h, int(pos.max()) // h
        tog = np.zeros((c1 - c0 + 1) * h, dtype=np.uint8)
        np.add.at(tog, pos - c0 * h, 1)                      # a few hundred crossings
        tog &= 1
        m[:, c0:c1 + 1] |= np.bitwise_xor.accumulate(tog).view(bool).reshape(c1 - c0 + 1, h).T
        if pos.size & 1:                      # an odd number of crossings: the last run of ones reaches the end of the canvas
            m[:, c1 + 1:] = True
    return m


def polygons_to_crossings(polygons, h, w):
    """The polygons of one instance as dgx_polygons_to_bitmask takes them (INPUT.DEVICE_RASTER): per polygon the crossings of
    polygon_crossings, those at or past h * w removed (a crossing clipped to the bottom of the last column), sorted ascending, int32.
    What polygons_to_bitmask does after this point -- toggle counts, the XOR scan, the transposed write -- is the kernel's."""
    out = []
    for poly in polygons:
        pos = polygon_crossings([float(c) for c in poly], h, w)
        out.append(np.sort(pos[pos < h * w]).astype(np.int32))
    return out


# ----------------------------------------------------------------------------------------------- mapper
def read_image(file_name, fmt="BGR"):
    """D2/data/detection_utils.py:read_image: PIL decode, EXIF orientation applied, RGB -> requested channel order."""
    from PIL import Image, ImageOps
    with open(file_name, "rb") as f:
        image = Image.open(f)
        image = ImageOps.exif_transpose(image)
        image = np.asarray(image.convert("RGB"))
    return image[:, :, ::-1] if fmt == "BGR" else image


def transform_instance_annotations(anno, transforms, image_size):
    """D2 transform_instance_annotations: XYWH -> XYXY box through the 4 corners, clipped; polygons point-wise."""
    x, y, bw, bh = anno["bbox"]
    corners = np.array([[x, y], [x + bw, y], [x, y + bh], [x + bw, y + bh]], dtype=np.float64)
    for t in transforms:
        corners = t.apply_coords(corners)
    box = np.concatenate([corners.min(0), corners.max(0)])
    anno["bbox"] = np.minimum(np.maximum(box, 0), np.array(list(image_size) + list(image_size))[::-1])
    anno["bbox_mode"] = "XYXY_ABS"
    if "segmentation" in anno:
        polys = []
        for p in anno["segmentation"]:
            c = np.asarray(p, dtype=np.float64).reshape(-1, 2)
            for t in transforms:
                c = t.apply_coords(c)
            polys.append(c.reshape(-1))
        anno["segmentation"] = polys
    return anno


def annotations_to_instances(annos, image_size, device_raster=False):
    """D2 annotations_to_instances with mask_format 'bitmask'.  device_raster (INPUT.DEVICE_RASTER): no (N, h, w) block is allocated
    or filled; gt_masks is a PolygonCrossings, the sorted crossing lists the training process fills on the device."""
    h, w = image_size
    target = Instances(image_size)
    boxes = np.stack([a["bbox"] for a in annos]) if annos else np.zeros((0, 4))
    target.gt_boxes = Boxes(torch.as_tensor(boxes, dtype=torch.float32).reshape(-1, 4))
    target.gt_classes = torch.tensor([int(a["category_id"]) for a in annos], dtype=torch.int64)
    if annos and "segmentation" in annos[0] and device_raster:
        target.gt_masks = PolygonCrossings.from_lists([polygons_to_crossings(a["segmentation"], h, w) for a in annos], image_size)
    elif annos and "segmentation" in annos[0]:
        masks = np.zeros((len(annos), h, w), dtype=bool)          # one contiguous block: it is pinned and uploaded as it is
        for i, a in enumerate(annos):
            polygons_to_bitmask(a["segmentation"], h, w, out=masks[i])
        target.gt_masks = BitMasks(torch.from_numpy(masks))
    return target


def filter_empty_instances(instances, box_threshold=1e-5):
    """D2 filter_empty_instances(by_box=True, by_mask=True)."""
    b = instances.gt_boxes.tensor
    keep = ((b[:, 2] - b[:, 0]) > box_threshold) & ((b[:, 3] - b[:, 1]) > box_threshold)
    if instances.has("gt_masks") and isinstance(instances.gt_masks, PolygonCrossings):
        keep &= instances.gt_masks.nonempty()          # emptiness from the crossings: equal to the filled mask's .any()
    elif instances.has("gt_masks"):
        gm = instances.gt_masks.tensor
        keep &= torch.from_numpy(gm.numpy().reshape(gm.shape[0], -1).any(1)) if not gm.is_cuda else gm.flatten(1).any(1)
    return instances[keep]


class DatasetMapper:
    """DG/divergen/data/dataset_mapper.py:127-256, training branch without proposals / keypoints / sem-seg."""

    def __init__(self, cfg, is_train=True, augmentations=None):
        self.is_train = is_train
        if augmentations is None:
            # training: DG/train_net.py:181-182 (custom augmentation); evaluation with TEST_INPUT_TYPE 'default': D2's own
            # mapper, i.e. ResizeShortestEdge(MIN_SIZE_TEST, MAX_SIZE_TEST) (DG/train_net.py:93-97)
            if is_train or cfg.INPUT.TEST_INPUT_TYPE != "default":
                augmentations = build_custom_augmentation(cfg, is_train)
            else:
                augmentations = [ResizeShortestEdge(cfg.INPUT.MIN_SIZE_TEST, cfg.INPUT.MAX_SIZE_TEST, "choice")]
        self.augmentations = augmentations
        # WITH_IMAGE_LABELS (DG custom_dataset_mapper.py:55-69, :108-117, :166-170): `ann_type` / `pos_category_ids` on every sample;
        # with USE_DIFF_BS_SIZE one EfficientDetResizeCrop per source
        self.with_ann_type = bool(cfg.WITH_IMAGE_LABELS)
        self.dataset_ann = list(cfg.DATALOADER.DATASET_ANN)
        self.dataset_augs = None
        if cfg.DATALOADER.USE_DIFF_BS_SIZE and is_train:       # (another CUSTOM_AUG: build_custom_augmentation has refused it above)
            self.dataset_augs = [[EfficientDetResizeCrop(size, tuple(scale)), RandomFlip()]
                                 for scale, size in zip(cfg.DATALOADER.DATASET_INPUT_SCALE, cfg.DATALOADER.DATASET_INPUT_SIZE)]
        self.image_format = cfg.INPUT.FORMAT
        self.use_instance_mask = cfg.MODEL.MASK_ON
        # INPUT.DEVICE_RASTER: the training samples carry their polygons' crossing lists instead of dense masks
        self.device_raster = bool(cfg.INPUT.get("DEVICE_RASTER", False)) and is_train
        # INPUT.DEVICE_RESIZE: the training samples carry the decoded source and the resize job instead of the mapped image
        self.device_resize = bool(cfg.INPUT.get("DEVICE_RESIZE", False)) and is_train
        if cfg.INPUT.MASK_FORMAT != "bitmask" and cfg.MODEL.MASK_ON and is_train:
            logger.warning("INPUT.MASK_FORMAT '%s': masks are rasterised to bitmasks on the loader side either way", cfg.INPUT.MASK_FORMAT)

    @staticmethod
    def _deferred_image(image, augs):
        """INPUT.DEVICE_RESIZE: the transforms are drawn exactly as in __call__ -- every get_transform sees an array-like of the shape the
        image would have at that point, and reads nothing else -- but no apply_image runs.  -> (DeviceResizeImage: the decoded source, the
        scaled size, the crop window, the flip and the window's coefficient tables; the transforms)."""
        from .resize_tables import ResizeJob

        class Shaped:
            def __init__(self, shape):
                self.shape = tuple(shape)
        transforms, cur, crop, flip = [], Shaped(image.shape), None, False
        for aug in augs:
            t = aug.get_transform(cur)
            if isinstance(t, EfficientDetResizeCropTransform) and crop is None and not flip:
                crop = t
                cur = Shaped((min(t.scaled_h, t.offset_y + t.target_size[0]) - t.offset_y,
                              min(t.scaled_w, t.offset_x + t.target_size[1]) - t.offset_x, image.shape[2]))
            elif isinstance(t, HFlipTransform):
                flip = not flip
            elif not isinstance(t, NoOpTransform):
                raise NotImplementedError("INPUT.DEVICE_RESIZE: the transform %s is not built for the device; one EfficientDetResizeCrop "
                                          "followed by RandomFlip is" % type(t).__name__)
            transforms.append(t)
        if crop is None:
            raise NotImplementedError("INPUT.DEVICE_RESIZE needs an EfficientDetResizeCrop among the augmentations")
        job = ResizeJob(image, (crop.scaled_h, crop.scaled_w), (crop.offset_y, crop.offset_x), cur.shape[:2], flip=flip)
        return DeviceResizeImage(job), transforms

    def __call__(self, dataset_dict):
        d = copy.deepcopy(dataset_dict)
        image = read_image(d["file_name"], self.image_format)
        if "width" in d and (d["width"], d["height"]) != (image.shape[1], image.shape[0]):
            raise ValueError("Mismatched image shape for {}: got {}, expect {}".format(
                d["file_name"], (image.shape[1], image.shape[0]), (d["width"], d["height"])))
        d.setdefault("width", image.shape[1])
        d.setdefault("height", image.shape[0])
        transforms = []
        augs = self.augmentations if self.dataset_augs is None else self.dataset_augs[d["dataset_source"]]
        if self.device_resize:
            d["image"], transforms = self._deferred_image(image, augs)
            image_shape = d["image"].shape[-2:]
        else:
            for aug in augs:
                t = aug.get_transform(image)
                image = t.apply_image(image)
                transforms.append(t)
            image_shape = image.shape[:2]
            d["image"] = torch.as_tensor(np.ascontiguousarray(image.transpose(2, 0, 1)))
        if not self.is_train:
            return d
        if "annotations" in d:
            annos = []
            for obj in d.pop("annotations"):
                if obj.get("iscrowd", 0) != 0:
                    continue
                if not self.use_instance_mask:
                    obj.pop("segmentation", None)
                annos.append(transform_instance_annotations(obj, transforms, image_shape))
            inst = filter_empty_instances(annotations_to_instances(annos, image_shape, self.device_raster))
            if not inst.has("gt_masks"):
                inst.gt_masks = BitMasks(torch.zeros(0, image_shape[0], image_shape[1], dtype=torch.bool))
            d["instances"] = inst
        if self.with_ann_type:
            d["pos_category_ids"] = d.get("pos_category_ids", [])
            d["ann_type"] = self.dataset_ann[d["dataset_source"]]
        return d


class CopyPasteMapper:
    """CopyPasteMapper.__call__ (mapper.py:856-958) for the shipped configuration: USE_COPY_METHOD 'syn_copy' with an instance
    pool -> InstPool.get_mix_result (divergen_amd/data/copypaste.py, pixels on the GPU compositor); the self-copy branch has
    no mix results in that configuration, so SimpleCopyPaste returns its input (custom_copypaste.py:254-259).
    USE_COPY_METHOD 'self_copy' / 'both' / 'p:<f>' (mapper.py:884-936): Simple Copy-Paste from a second training image
    (custom_copypaste.py:242-341), worker half in _call_self_copy, pixels in dgx_self_copy_paste (_finish_self_copy); with
    INPUT.SCP_MULTI_SRC from INPUT.SCP_NUM_SRC <= 4 images, merged by dgx_self_copy_merge first.
    With INPUT.SCP_SRC_MODES: INPUT.SCP_TYPE 'in_domain' / 'cas' / 'the_cls' / 'the_cls_img' (mapper.py:782-815, :829-835: the source
    drawn per category, _class_sources), a source pasted whole (mapper.py:764-765: dgx_self_copy_paste_all) and INPUT.RM_BG_PROB
    (mapper.py:869-872, under every copy method: dgx_remove_background in finish)."""

    SCP_TYPES = ("in_domain", "cas", "the_cls", "the_cls_img")
    # what INPUT.SCP_SRC_MODES switches on; the defaults are what a mapper without the key does
    scp_type, paste_all, rm_bg_prob, per_cat_map, select_cats = "", False, 0.0, None, ()

    def __init__(self, mapper, cfg):
        self.mapper = mapper
        self.use_scp = cfg.INPUT.USE_SCP
        self.num_src = cfg.INPUT.SCP_NUM_SRC
        self.method = cfg.INPUT.USE_COPY_METHOD
        self.src_modes = bool(cfg.INPUT.get("SCP_SRC_MODES", False))
        self.inst_pool = None
        self.dataset = None
        self.pack = True               # one blob per sample across the process boundary (pack_sample); the loader's finish() unpacks
        self.ring = None               # SlotRing the workers wrote the blobs into (build_detection_train_loader)
        self.self_prob = self._parse_method(self.method)      # None: no self copy; 1.0: always; f: 'p:<f>', per sample
        self.self_only = self.method == "self_copy"
        self.device_raster = bool(cfg.INPUT.get("DEVICE_RASTER", False))
        if self.device_raster:
            self._check_device_raster(cfg)
        self.device_resize = bool(cfg.INPUT.get("DEVICE_RESIZE", False))
        if self.device_resize:
            self._check_device_resize(cfg)
        if self.self_prob is not None:
            self._check_self_copy(cfg)
        if self.src_modes:
            self._check_rm_bg(cfg)
            self.rm_bg_prob = max(float(cfg.INPUT.RM_BG_PROB), 0.0)
            if self.self_prob is not None:
                self.scp_type, self.select_cats = cfg.INPUT.SCP_TYPE, list(cfg.INPUT.SCP_SELECT_CATS_LIST)
                self.paste_all = self._pastes_all(cfg.INPUT) is not None
        if cfg.INPUT.INST_POOL and self.method != "none" and not self.self_only:
            from .copypaste import InstPool
            if cfg.INPUT.INST_POOL_SAMPLE_TYPE != "cas_random" or cfg.INPUT.INST_POOL_FORMAT != "RGBA":
                raise NotImplementedError("only INST_POOL_FORMAT 'RGBA' with INST_POOL_SAMPLE_TYPE 'cas_random' is built")
            self.inst_pool = InstPool.from_config(cfg)
            self.inst_pool.device_resize = self.device_resize

        # BSGAL (BS/bsgal/data/custom_build_copypaste_mapper.py:237-297, :916-930, :958-963, :1038-1057): keep the un-pasted
        # sample and add a held-out image that shows one of the pasted classes
        self.active_select = bool(cfg.INPUT.get("ACTIVE_SELECT", False))
        self.active_test = cfg.MODEL.get("ACTIVE_TEST", "select")
        self.active_test_one = cfg.MODEL.get("ACTIVE_TEST_INS", "one") == "one" and "one_class" in cfg.INPUT.INST_POOL_SAMPLE_TYPE
        self.per_cat_pool_real = None

    @staticmethod
    def _parse_method(method):
        """INPUT.USE_COPY_METHOD (mapper.py:884-890) -> probability of the self-copy branch per sample (None: never taken)."""
        if method in ("none", "syn_copy"):
            return None
        if method in ("self_copy", "both"):
            return 1.0
        if isinstance(method, str) and method.startswith("p:"):
            try:
                f = float(method[2:])
            except ValueError:
                f = float("nan")
            if not 0.0 <= f <= 1.0:
                raise ValueError("INPUT.USE_COPY_METHOD '{}': 'p:<f>' needs a probability in [0, 1]".format(method))
            return f
        raise NotImplementedError("INPUT.USE_COPY_METHOD '{}': 'none', 'syn_copy', 'self_copy', 'both' and 'p:<f>' are built".format(method))

    @staticmethod
    def _check_self_copy(cfg):
        """The self-copy branch is built for SCP_TYPE '', one source image (up to SELF_COPY_MAX_SRC with this build's key
        INPUT.SCP_MULTI_SRC), selected objects, 'basic' blend (the reference's own choice, mapper.py:770); every other switch of that
        branch is refused by name.  This build's key INPUT.SCP_SRC_MODES admits SCP_TYPE 'in_domain' / 'cas' / 'the_cls' /
        'the_cls_img', SCP_SRC_OBJ_SELECT False and RM_BG_PROB in (0, 1] (_check_src_modes, _check_rm_bg)."""
        from ..layers.copy_paste import SELF_COPY_MAX_SRC
        inp = cfg.INPUT
        modes = bool(inp.get("SCP_SRC_MODES", False))
        if modes:
            CopyPasteMapper._check_src_modes(cfg)
        if bool(inp.get("SCP_MULTI_SRC", False)) and not 1 <= inp.SCP_NUM_SRC <= SELF_COPY_MAX_SRC:
            raise NotImplementedError("INPUT.SCP_NUM_SRC {!r} with INPUT.USE_COPY_METHOD '{}': INPUT.SCP_MULTI_SRC merges 1 to {} source "
                                      "images (dgx_self_copy_merge)".format(inp.SCP_NUM_SRC, inp.USE_COPY_METHOD, SELF_COPY_MAX_SRC))
        refused = [("SCP_TYPE", inp.SCP_TYPE != "" and not modes, "only '' (a random training image as the source)"),
                   ("SCP_NUM_SRC", inp.SCP_NUM_SRC != 1 and not bool(inp.get("SCP_MULTI_SRC", False)),
                    "only 1 (several sources are merged on a temporary canvas first)"),
                   ("SCP_SRC_OBJ_SELECT", not inp.SCP_SRC_OBJ_SELECT and not modes, "only True"),
                   ("BLANK_RATIO", inp.BLANK_RATIO > 0, "the source is not resized (needs cv2.resize)"),
                   ("ROTATE_SRC", bool(inp.ROTATE_SRC), "the source is not rotated"),
                   ("LIMIT_SRC_LSJ", bool(inp.LIMIT_SRC_LSJ), "the source takes the mapper's default augmentations"),
                   ("RM_BG_PROB", inp.RM_BG_PROB > 0 and not modes, "background removal is not built"),
                   ("SCP_RFS", bool(inp.SCP_RFS), "the source index is drawn uniformly"),
                   ("USE_INSTABOOST", bool(inp.USE_INSTABOOST), "InstaBoost is not built"),
                   ("USE_COLOR_JITTER", bool(inp.USE_COLOR_JITTER), "colour jitter is not built")]
        for key, bad, why in refused:
            if bad:
                raise NotImplementedError("INPUT.{} {!r} with INPUT.USE_COPY_METHOD '{}': {}".format(key, inp[key], inp.USE_COPY_METHOD, why))
        if bool(inp.get("ACTIVE_SELECT", False)):
            raise NotImplementedError("INPUT.ACTIVE_SELECT with INPUT.USE_COPY_METHOD '{}': BSGAL's origin / held-out samples are built "
                                      "for 'syn_copy' only".format(inp.USE_COPY_METHOD))

    @staticmethod
    def _check_device_raster(cfg):
        """This build's key INPUT.DEVICE_RASTER is built for USE_COPY_METHOD 'none' and 'syn_copy' (with or without RM_BG_PROB under
        INPUT.SCP_SRC_MODES, WITH_IMAGE_LABELS): there the masks are first read on the device.  The self-copy methods read the source's
        masks in the WORKER (_call_self_copy selects and crops them), and BSGAL's held-out sample is indexed by class there."""
        inp = cfg.INPUT
        if CopyPasteMapper._parse_method(inp.USE_COPY_METHOD) is not None:
            raise NotImplementedError("INPUT.DEVICE_RASTER with INPUT.USE_COPY_METHOD '{}': the self-copy methods read the source image's "
                                      "masks in the loader worker; 'none' and 'syn_copy' are built".format(inp.USE_COPY_METHOD))
        if bool(inp.get("ACTIVE_SELECT", False)):
            raise NotImplementedError("INPUT.DEVICE_RASTER with INPUT.ACTIVE_SELECT: BSGAL's origin / held-out samples are built on dense "
                                      "host masks")

    @staticmethod
    def _check_device_resize(cfg):
        """This build's key INPUT.DEVICE_RESIZE is built for USE_COPY_METHOD 'none' and 'syn_copy' (with or without INPUT.DEVICE_RASTER,
        RM_BG_PROB under INPUT.SCP_SRC_MODES, WITH_IMAGE_LABELS, USE_DIFF_BS_SIZE): there the pixels are first read on the device.  The
        self-copy methods crop the source image's pixels in the WORKER (_call_self_copy), and BSGAL's held-out image stays on the host."""
        inp = cfg.INPUT
        if CopyPasteMapper._parse_method(inp.USE_COPY_METHOD) is not None:
            raise NotImplementedError("INPUT.DEVICE_RESIZE with INPUT.USE_COPY_METHOD '{}': the self-copy methods read the source image's "
                                      "pixels in the loader worker; 'none' and 'syn_copy' are built".format(inp.USE_COPY_METHOD))
        if bool(inp.get("ACTIVE_SELECT", False)):
            raise NotImplementedError("INPUT.DEVICE_RESIZE with INPUT.ACTIVE_SELECT: BSGAL's held-out image is mapped and kept on the host")

    @staticmethod
    def _pastes_all(inp):
        """The key that makes the source paste whole -- CopyPaste(selected=SCP_SRC_OBJ_SELECT and scp_type not in ('in_domain', 'cas')),
        mapper.py:764-765 -- or None when _select_object runs."""
        if inp.SCP_TYPE in ("in_domain", "cas"):
            return "SCP_TYPE"
        return None if inp.SCP_SRC_OBJ_SELECT else "SCP_SRC_OBJ_SELECT"

    @staticmethod
    def _check_src_modes(cfg):
        """What INPUT.SCP_SRC_MODES still refuses of the switches it admits to a self-copy method."""
        inp = cfg.INPUT
        t = inp.SCP_TYPE
        if t in ("rc_only", "f_only"):
            raise NotImplementedError("INPUT.SCP_TYPE {!r} with INPUT.USE_COPY_METHOD '{}': the reference's own mapper has no branch for it "
                                      "and raises NotImplementedError at the first sample (mapper.py:892-916); INPUT.SCP_SRC_MODES builds "
                                      "'', {}".format(t, inp.USE_COPY_METHOD, ", ".join(repr(x) for x in CopyPasteMapper.SCP_TYPES)))
        if t != "" and t not in CopyPasteMapper.SCP_TYPES:
            raise NotImplementedError("INPUT.SCP_TYPE {!r} with INPUT.USE_COPY_METHOD '{}': INPUT.SCP_SRC_MODES builds '', {}".format(
                t, inp.USE_COPY_METHOD, ", ".join(repr(x) for x in CopyPasteMapper.SCP_TYPES)))
        if t in ("the_cls", "the_cls_img") and len(inp.SCP_SELECT_CATS_LIST) < max(int(inp.SCP_NUM_SRC), 1):
            raise ValueError("INPUT.SCP_SELECT_CATS_LIST {!r} with INPUT.SCP_TYPE {!r}: INPUT.SCP_NUM_SRC {} categories are drawn from it "
                             "without replacement per sample".format(list(inp.SCP_SELECT_CATS_LIST), t, inp.SCP_NUM_SRC))
        whole = CopyPasteMapper._pastes_all(inp)
        if whole is not None and inp.SCP_NUM_SRC > 1:
            raise NotImplementedError("INPUT.SCP_NUM_SRC {!r} with INPUT.{} {!r}: a source pasted whole is built for one source image "
                                      "(dgx_self_copy_merge takes at most 99 objects per source)".format(inp.SCP_NUM_SRC, whole, inp[whole]))

    @staticmethod
    def _check_rm_bg(cfg):
        """INPUT.RM_BG_PROB under INPUT.SCP_SRC_MODES, whatever the copy method (the reference draws it before `if self.use_scp`)."""
        inp = cfg.INPUT
        if inp.RM_BG_PROB > 1:
            raise ValueError("INPUT.RM_BG_PROB {!r}: a probability, at most 1 (the reference asserts it at the first sample, "
                             "mapper.py:870)".format(inp.RM_BG_PROB))
        if inp.RM_BG_PROB > 0 and bool(inp.get("ACTIVE_SELECT", False)):
            raise NotImplementedError("INPUT.RM_BG_PROB {!r} with INPUT.ACTIVE_SELECT: background removal is built for DiverGen's mapper; "
                                      "BSGAL's is a different file".format(inp.RM_BG_PROB))

    def set_dataset(self, dataset):
        self.dataset = dataset
        if self.scp_type in self.SCP_TYPES:
            # mapper.py:829-835: image indices per category, categories in order of first appearance ('cas' draws from the keys)
            self.per_cat_map = {}
            for i, d in enumerate(dataset):
                for cid in set([a["category_id"] for a in d.get("annotations", [])]):
                    self.per_cat_map.setdefault(cid, []).append(i)
            if self.scp_type == "cas" and len(self.per_cat_map) < self.num_src:
                raise ValueError("INPUT.SCP_TYPE 'cas' with INPUT.SCP_NUM_SRC {}: the training set shows {} categories".format(
                    self.num_src, len(self.per_cat_map)))
        if self.active_select:
            pool = {}
            for i, d in enumerate(dataset):
                for a in d.get("annotations", []):
                    pool.setdefault(a["category_id"], set()).add(i)
            self.per_cat_pool_real = {k: sorted(v) for k, v in pool.items()}

    def _held_out(self, paste_labels, own_labels):
        """The test image of one sample (:260-284): a class among the pasted ones ('select'), else among the image's own,
        else any; re-drawn until some training image shows it; then one of those images through the plain mapper."""
        ncls = 1203
        if not any(self.per_cat_pool_real.values()):
            raise ValueError("INPUT.ACTIVE_SELECT needs a training set with annotations: no category has an image to hold out")
        if self.active_test == "select":
            cand = sorted(set(paste_labels)) or sorted(set(own_labels))
            cls = int(np.random.choice(cand)) if cand else int(np.random.choice(range(ncls)))
        else:
            cls = int(np.random.choice(range(ncls)))
        while not self.per_cat_pool_real.get(cls):
            cls = int(np.random.choice(range(ncls)))
        pool = self.per_cat_pool_real[cls]
        idx = pool[np.random.randint(0, len(pool))]
        if self.active_test == "random_img":
            idx = np.random.randint(0, len(self.dataset))
        test = self.mapper(self.dataset[idx])
        if self.active_test_one:
            test["instances"] = test["instances"][test["instances"].gt_classes == cls]
        return cls, test

    def __call__(self, dataset_dict):
        """What a LOADER WORKER runs -- all of CopyPasteMapper.__call__ (mapper.py:856-958) except the pixel blend: decode +
        augment + rasterise, the self-copy index draw (:877), the instance pool's draws / decode / largest component / resize /
        flip / placement packed for the compositor (InstPool.prepare), BSGAL's held-out image.  CPU tensors only."""
        result = self.mapper(dataset_dict)
        if "instances" not in result or not result["instances"].has("gt_masks"):        # mapper.py:862-864
            return result
        if result.get("ann_type", "box") != "box":
            # an image-labelled sample: in the reference it has no annotations, hence no gt_masks, and leaves at :862-864 before any
            # draw; here it carries EMPTY instances (with an empty mask stack), so it leaves by its annotation type
            return result
        if self.rm_bg_prob > 0 and np.random.uniform(0.0, 1.0) <= self.rm_bg_prob:      # mapper.py:869-872; the pixels: finish()
            result = dict(result, rm_bg=True)
        idxs = []
        if self.use_scp and self.dataset is not None:
            idxs = [np.random.randint(0, len(self.dataset)) for _ in range(self.num_src)]
        if self.self_prob is not None and idxs:
            return self._call_self_copy(result, idxs)
        if self.inst_pool is None:
            return result
        result = self.inst_pool.prepare(result)
        if self.active_select:
            cls, test = self._held_out(result.get("paste_labels", []), result["instances"].gt_classes.tolist())
            result["test_image"], result["test_instances"] = test["image"], test["instances"]
            result["test_image_class"], result["test_file_name"] = cls, test.get("file_name")
        return pack_sample(result) if self.pack else result

    def _call_self_copy(self, result, idxs):
        """The self-copy methods (mapper.py:884-936 + CopyPaste._select_object, custom_copypaste.py:393-411), worker half, in the
        reference's np.random order: [rand() for 'p:<f>'] -> the source images through the same mapper, in index order (each its own
        resize-crop and flip draws) -> the instance pool's draws when the sample takes the pool branch -> per source, in order,
        m = randint(0, min(ns + 1, 100)), sel = choice(ns, m, replace=False).  Adds `scp_src`: the source image, the m selected
        masks / boxes / labels in paste order and the canvas size -- what dgx_self_copy_paste needs; the training process runs it
        (finish).  With INPUT.SCP_NUM_SRC > 1 the sources that selected nothing are skipped as the reference skips them; one left is
        the case above, byte for byte; two or more make `scp_src` a LIST of such groups (no canvas: it follows from the merge), each
        cropped to the largest box extent of all of them, beyond which no stage's canvas reaches.
        INPUT.SCP_SRC_MODES: the sources of an INPUT.SCP_TYPE come from _class_sources instead (the index draws above stay consumed,
        :877); a source pasted whole makes no selection draw and ships all its objects in their order, marked `all` for finish; no source
        at all ('in_domain' on a destination without instances) leaves the sample without `scp_src`: CopyPaste.__call__ returns its
        input untouched then (custom_copypaste.py:257-259), Instances not rebuilt."""
        from ..layers.copy_paste import self_copy_canvas
        take_self, take_syn = True, self.method == "both"
        if self.method.startswith("p:"):
            take_self = np.random.rand() < self.self_prob
            take_syn = not take_self
        if not take_self:
            srcs = []
        elif self.scp_type == "":
            srcs = [self.mapper(self.dataset[i]) for i in idxs]
        else:
            srcs = self._class_sources(result)
        if take_syn and self.inst_pool is not None:
            result = self.inst_pool.prepare(result)
        if take_self and srcs:
            result = dict(result)
            picked = []                                        # (source, selected indices) of the sources that selected something
            for src in srcs:
                ns = len(src["instances"])
                if self.paste_all:                             # CopyPaste(selected=False): no draw
                    m, sel = ns, np.arange(ns)
                else:
                    m = np.random.randint(0, min(ns + 1, 100))
                    sel = np.random.choice(ns, size=m, replace=False)
                if m:
                    picked.append((src, torch.from_numpy(np.asarray(sel, dtype=np.int64))))
            h1, w1 = result["image"].shape[-2:]

            def group(src, sel_t, H, W):
                # only what the canvas can show travels: the source cropped to (H, W) (the kernel zero-pads a smaller one)
                si = src["instances"]
                return {"image": src["image"][:, :H, :W].contiguous(),
                        "masks": si.gt_masks.tensor.view(torch.uint8)[sel_t][:, :H, :W].contiguous(),
                        "boxes": si.gt_boxes.tensor[sel_t].contiguous(), "labels": si.gt_classes[sel_t].contiguous()}
            if len(picked) == 1:
                src, sel_t = picked[0]
                H, W = self_copy_canvas((h1, w1), src["instances"].gt_boxes.tensor[sel_t])
                result["scp_src"] = dict(group(src, sel_t, H, W), hw=(H, W))
                if self.paste_all:
                    result["scp_src"]["all"] = True
            elif picked:
                H, W = self_copy_canvas((0, 0), torch.cat([src["instances"].gt_boxes.tensor[sel_t] for src, sel_t in picked]))
                result["scp_src"] = [group(src, sel_t, H, W) for src, sel_t in picked]
            else:                                          # nothing pasted; the Instances is still rebuilt (custom_copypaste.py:311-318)
                result["scp_src"] = {"image": torch.zeros(3, 0, 0, dtype=torch.uint8), "masks": torch.zeros(0, 0, 0, dtype=torch.uint8),
                                     "boxes": torch.zeros(0, 4), "labels": torch.zeros(0, dtype=torch.int64), "hw": (int(h1), int(w1))}
            if self.inst_pool is not None and picked:
                # blend_image's `random.sample(['basic'], 1)` (custom_copypaste.py:467), once per _copy_paste that happens: the
                # len(picked) - 1 temporary stages and the final paste
                self.inst_pool.draw_modes(len(picked))
            result["scp_file_name"] = srcs[0].get("file_name") if len(srcs) == 1 else [src.get("file_name") for src in srcs]
        return pack_sample(result) if self.pack else result

    def _class_sources(self, result):
        """_filter_in_specific_cls (mapper.py:782-815) in its np.random order: the categories -- 'in_domain': num_src draws among the
        destination's own classes (none: no source, no draw); 'cas' / 'the_cls*': choice without replacement among the categories of the
        training set / INPUT.SCP_SELECT_CATS_LIST -- then per source one image of that category's list, a deep copy of its dict with the
        annotations filtered to the class list (not for 'the_cls_img'), through the mapper with its own draws."""
        t = self.scp_type
        if t == "in_domain":
            cls_list = list(set(result["instances"].gt_classes.tolist()))
            cats_pool = [self.per_cat_map.get(c, []) for c in cls_list]
            if len(cats_pool) == 0:
                return []
            pools = [cats_pool[np.random.randint(0, len(cats_pool))] for _ in range(self.num_src)]
        else:
            cls_list = np.random.choice(list(self.per_cat_map.keys()) if t == "cas" else self.select_cats, self.num_src, replace=False)
            pools = [self.per_cat_map.get(c, []) for c in cls_list]
        srcs = []
        for pool in pools:
            d = copy.deepcopy(self.dataset[pool[np.random.randint(0, len(pool))]])
            if t != "the_cls_img":
                d["annotations"] = [a for a in d["annotations"] if a["category_id"] in cls_list]
            srcs.append(self.mapper(d))
        return srcs

    @staticmethod
    def _finish_self_copy(out, scp, dev):
        """Training-process half of the self copy: ONE dgx_self_copy_paste call on the current stream (a list of source groups:
        layers.self_copy_paste_multi -- dgx_self_copy_merge, one read-back, dgx_self_copy_paste_merged), then the Instances rebuilt with
        gt_boxes / gt_classes / gt_masks only (custom_copypaste.py:311-318: instance_source and every other field are gone, also
        when nothing was pasted).  A source pasted whole (`all`): dgx_self_copy_paste_all, any number of objects."""
        from ..layers.copy_paste import self_copy_paste, self_copy_paste_all, self_copy_paste_multi
        from .copypaste import result_instances
        if dev.type != "cuda":
            raise RuntimeError("INPUT.USE_COPY_METHOD with a self copy needs the GPU compositor (dgx_self_copy_paste); device is %s" % dev)
        inst = out["instances"]
        up = lambda t: t.to(dev, non_blocking=True)     # noqa: E731
        dst = (out["image"], inst.gt_masks.tensor.view(torch.uint8), inst.gt_boxes.tensor, inst.gt_classes)
        if isinstance(scp, list):      # several sources (INPUT.SCP_MULTI_SRC): dgx_self_copy_merge, one read-back, then the paste
            r = self_copy_paste_multi(*dst, [tuple(up(g[k]) for k in ("image", "masks", "boxes", "labels")) for g in scp], lazy_masks=True)
        elif scp.get("all"):
            r = self_copy_paste_all(*dst, up(scp["image"]), up(scp["masks"]), up(scp["boxes"]), up(scp["labels"]), canvas_hw=scp["hw"],
                                    lazy_masks=True)
        else:
            m = int(scp["labels"].shape[0])
            r = self_copy_paste(*dst, up(scp["image"]), up(scp["masks"]), up(scp["boxes"]), up(scp["labels"]), np.arange(m),
                                canvas_hw=scp["hw"], lazy_masks=True)
        out["instances"] = result_instances(r, with_source=False)
        out["image"], (out["height"], out["width"]) = r["image"], out["instances"].image_size
        return out

    @staticmethod
    def _finish_rm_bg(result, dev, own):
        """Training-process half of INPUT.RM_BG_PROB (mapper.py:869-872): the image and the masks go up and ONE dgx_remove_background
        call on the current stream blanks what no mask covers -- before the pool compositor and the self copy, which then find both on
        the device.  own: the uploaded image is this call's own copy and is rewritten in place."""
        from ..layers.copy_paste import remove_background
        if dev.type != "cuda":
            raise RuntimeError("INPUT.RM_BG_PROB needs the GPU kernel (dgx_remove_background); device is %s" % dev)
        result = {k: v for k, v in result.items() if k != "rm_bg"}
        own = own or not result["image"].is_cuda
        image, inst = result["image"].to(dev, non_blocking=True), result["instances"].to(dev)
        result["image"] = remove_background(image, inst.gt_masks.tensor.view(torch.uint8), out=image if own and image.is_contiguous() else None)
        result["instances"] = inst
        return result

    def finish(self, result, device):
        """What the TRAINING PROCESS runs on one worker result, on the current stream: upload (asynchronous from pinned memory) and
        the compositor kernel; with INPUT.ACTIVE_SELECT the un-pasted sample stays available as origin_* (it is the uploaded
        input: the compositor writes a copy)."""
        from .copypaste import InstPool, fill_device_masks, materialize_resizes
        dev = torch.device(device)
        own = "blob" in result                       # the sample's tensors come out of a device copy made here
        result = unpack_sample(result, dev, self.ring)
        if isinstance(result.get("image"), DeviceResizeImage):
            result = materialize_resizes(result, dev)    # INPUT.DEVICE_RESIZE: first, on every exit; the image is this call's own tensor
            own = True
        if "instances" not in result:
            result["image"] = result["image"].to(dev, non_blocking=True)
            return result
        result = fill_device_masks(result, dev)      # INPUT.DEVICE_RASTER: from here on the sample is what the key-off path carries
        if result.get("rm_bg"):
            result = self._finish_rm_bg(result, dev, own)
        if "paste_pack" in result and dev.type == "cuda":
            out = InstPool.composite(result, dev)
            img, gm, gb, gc = out.pop("_uploaded")
            origin = Instances(tuple(img.shape[-2:]), gt_boxes=Boxes(gb), gt_classes=gc, gt_masks=BitMasks(gm.view(torch.bool)))
        else:
            out = {k: v for k, v in result.items() if k != "paste_pack"}
            out["image"], out["instances"] = out["image"].to(dev, non_blocking=True), out["instances"].to(dev)
            img, origin = out["image"], out["instances"]
        scp = out.pop("scp_src", None)
        if scp is not None:
            out = self._finish_self_copy(out, scp, dev)
        if self.active_select and "test_image" in out:
            out["origin_image"], out["origin_instances"] = img, origin
            if not origin.has("instance_source"):
                origin.instance_source = torch.zeros(len(origin), dtype=torch.int64, device=dev)
            out["test_image"], out["test_instances"] = out["test_image"].to(dev, non_blocking=True), out["test_instances"].to(dev)
        return out


# ---- one blob per sample.  A worker result used to cross the process boundary as 7 tensors per image (image, masks, boxes, classes,
# paste patches, paste descriptors, paste labels): 7 shared-memory segments whose file descriptors are handed over one authenticated
# socket round trip each (Python, under the GIL, in the training process's pin thread), 7 pinned copies, 7 host -> device copies issued
# by the training thread.  The worker now lays them out in ONE uint8 tensor (sections 64-byte aligned) + a small layout list; the
# training process pins and uploads that one tensor and takes the fields as VIEWS of the device copy.
_BLOB_FIELDS = (("image", lambda d: d["image"]), ("gt_masks", lambda d: d["instances"].gt_masks.tensor.view(torch.uint8)),
                ("gt_boxes", lambda d: d["instances"].gt_boxes.tensor), ("gt_classes", lambda d: d["instances"].gt_classes),
                ("flat", lambda d: d["paste_pack"]["flat"]), ("desc", lambda d: d["paste_pack"]["desc"]), ("labels", lambda d: d["paste_pack"]["labels"]))


def _blob_scp_sections(prefix):
    """The four optional sections of one self-copy source (CopyPasteMapper._call_self_copy) as (section name, key in the source's
    dict): prefix "scp_" for the single source, "scp%d_" % i for group i of a sample whose scp_src is a LIST (INPUT.SCP_NUM_SRC > 1,
    two or more sources selected something)."""
    return tuple((prefix + k, k) for k in ("image", "masks", "boxes", "labels"))


def pack_sample(d):
    """Worker side: the sample's tensors -> d['blob'] (uint8) + d['blob_layout'] [(name, dtype, shape, byte offset)]; the tensor
    entries themselves are dropped.  Samples without paste_pack / instances pass through unchanged.  Sections: the four of the
    sample, the three of paste_pack when it has one, the four of the self-copy source (scp_src) when it has one -- four per group
    when scp_src is a list of source groups, counted by blob_scp_n; a sample without scp_src, and one with a single source, pack
    exactly as they always did.  INPUT.DEVICE_RASTER: the instances' gt_masks is a PolygonCrossings, and the sections poly_pos (int32),
    poly_off and inst_off (int64) stand where gt_masks would.  INPUT.DEVICE_RESIZE: the image is a DeviceResizeImage, and the sections
    rs_src (uint8), rs_jobs (int32 (J, 13)) and rs_tab (int32) stand where image would; `flat` keeps the ranges of the patches left to
    the device unwritten."""
    if ("paste_pack" not in d and "scp_src" not in d) or "instances" not in d or not d["instances"].has("gt_masks"):
        return d
    fields = _BLOB_FIELDS if "paste_pack" in d else _BLOB_FIELDS[:4]
    gm = d["instances"].gt_masks
    if isinstance(gm, PolygonCrossings):      # INPUT.DEVICE_RASTER: three small sections in place of gt_masks
        fields = fields[:1] + tuple((name, lambda d, a=a: torch.from_numpy(a)) for name, a in
                                    (("poly_pos", gm.pos), ("poly_off", gm.poly_off), ("inst_off", gm.inst_off))) + fields[2:]
    if isinstance(d["image"], DeviceResizeImage):
        # INPUT.DEVICE_RESIZE: the sources (the image's, then those of the pool patches left to the device), the job table and the
        # coefficient tables of the sample's ONE resize launch stand where the image would
        from .resize_tables import assemble_jobs
        left = d["paste_pack"].get("resize", ()) if "paste_pack" in d else ()
        rs = assemble_jobs([d["image"].job] + [job for job, _ in left], [0] + [off for _, off in left])
        fields = tuple((name, lambda d, a=a: torch.from_numpy(a)) for name, a in zip(("rs_src", "rs_jobs", "rs_tab"), rs)) + fields[1:]
    multi = isinstance(d.get("scp_src"), list)
    groups = []
    if multi:
        groups = [("scp%d_" % i, g) for i, g in enumerate(d["scp_src"])]
    elif "scp_src" in d:
        groups = [("scp_", d["scp_src"])]
    for prefix, g in groups:
        fields = fields + tuple((name, lambda d, g=g, k=k: g[k]) for name, k in _blob_scp_sections(prefix))
    parts, layout, off = [], [], 0
    for name, get in fields:
        t = get(d).contiguous()
        raw = t.view(-1).view(torch.uint8) if t.numel() else torch.zeros(0, dtype=torch.uint8)
        layout.append((name, str(t.dtype).replace("torch.", ""), tuple(t.shape), off))
        pad = (-raw.numel()) % 64
        parts.append(raw)
        if pad:
            parts.append(torch.zeros(pad, dtype=torch.uint8))
        off += raw.numel() + pad
    out = {k: v for k, v in d.items() if k not in ("image", "instances", "paste_pack", "scp_src")}
    out["blob"], out["blob_layout"] = torch.cat(parts) if parts else torch.zeros(0, dtype=torch.uint8), layout
    out["blob_hw"] = tuple(d["image"].shape[-2:])
    if multi:
        out["blob_scp_n"] = len(d["scp_src"])
    elif "scp_src" in d:
        out["blob_scp_hw"] = tuple(int(v) for v in d["scp_src"]["hw"])
        if d["scp_src"].get("all"):                  # a source pasted whole (INPUT.SCP_SRC_MODES): finish calls dgx_self_copy_paste_all
            out["blob_scp_all"] = True
    if "paste_pack" in d:
        out["blob_K"] = int(d["paste_pack"]["K"])
    modes = d["paste_pack"].get("modes") if "paste_pack" in d else None
    if modes is not None and np.asarray(modes).any():
        # K blend-mode bytes, read by the host when it launches the compositor (so not in the blob), as a numpy array: it pickles
        # inline, where a tensor would cost the training thread a shared-memory handle round trip.  All 'basic' (the shipped
        # configs): nothing is added, the sample crosses the queue exactly as before.
        from ..layers.copy_paste import POISSON
        out["blob_modes"] = np.ascontiguousarray(modes, dtype=np.uint8)
        if (out["blob_modes"] == POISSON).any():
            # a 'possion' paste (INPUT.CP_POISSON): the compositor sizes the solver's workspace from the paste's rectangle, on the
            # host -- the K descriptors travel once more next to the modes (they are also in the blob, for the device)
            out["blob_desc"] = np.ascontiguousarray(d["paste_pack"]["desc"].numpy(), dtype=np.int32).reshape(-1, 5)
    extra = {k: v for k, v in d["instances"].get_fields().items() if k not in ("gt_masks", "gt_boxes", "gt_classes")}
    if extra:
        out["blob_extra_fields"] = extra
    return out


def unpack_sample(d, device, ring=None):
    """Training-process side: d['blob'] (or the slot of the page-locked ring it was written into) goes to `device` in ONE asynchronous
    copy; image / instances / paste_pack come back as views of it."""
    if "blob" not in d:
        return d
    if d.get("blob_slot") is not None:
        from .. import _lib as L
        off, n = d["blob_slot"]
        host = ring.buf[off:off + n]
        blob = torch.empty(n, dtype=torch.uint8, device=device)
        L.check(L.lib().dgx_memcpy_h2d_async(blob.data_ptr(), ring.buf.data_ptr() + off, n, L.stream()), "dgx_memcpy_h2d_async")
    else:
        host = d["blob"]
        blob = host.to(device, non_blocking=True)
    f = {}
    for name, dt, shape, off in d["blob_layout"]:
        dtype = getattr(torch, dt)
        n = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
        f[name] = blob[off:off + n].view(dtype).view(shape)
    out = {k: v for k, v in d.items() if not k.startswith("blob")}
    # INPUT.DEVICE_RASTER / DEVICE_RESIZE: offsets and tables are validated on the host before a kernel indexes with them -- read from
    # the host side of the blob (a copy: the slot is rewritten later), while the kernel reads the sections of the device copy
    sec = {name: (dt, shape, off) for name, dt, shape, off in d["blob_layout"]}

    def on_host(name):
        dt, shape, off = sec[name]
        a = np.dtype(dt)
        return host[off:off + int(np.prod(shape)) * a.itemsize].numpy().view(a).copy().reshape(shape)
    if "rs_src" in f:
        jobs_host = on_host("rs_jobs")               # job 0 is the image: word 3 is its channel count
        out["image"] = DeviceResizeImage(shape=(int(jobs_host[0, 3]),) + tuple(d["blob_hw"]),
                                         pending={"src": f["rs_src"], "jobs": f["rs_jobs"], "tab": f["rs_tab"],
                                                  "jobs_host": jobs_host, "tab_host": on_host("rs_tab")})
    else:
        out["image"] = f["image"]
    if "poly_pos" in f:
        masks = PolygonCrossings(on_host("poly_pos"), on_host("poly_off"), on_host("inst_off"), tuple(d["blob_hw"]),
                                 device_copy=(f["poly_pos"], f["poly_off"], f["inst_off"]))
    else:
        masks = BitMasks(f["gt_masks"].view(torch.bool))
    inst = Instances(tuple(d["blob_hw"]), gt_boxes=Boxes(f["gt_boxes"]), gt_classes=f["gt_classes"], gt_masks=masks)
    for k, v in d.get("blob_extra_fields", {}).items():
        inst.set(k, v.to(device) if hasattr(v, "to") else v)
    out["instances"] = inst
    if "flat" in f:
        out["paste_pack"] = {"flat": f["flat"], "desc": f["desc"], "labels": f["labels"], "K": d["blob_K"]}
        if d.get("blob_modes") is not None:
            out["paste_pack"]["modes"] = d["blob_modes"]
        if d.get("blob_desc") is not None:
            out["paste_pack"]["desc_host"] = d["blob_desc"]
    if "scp_image" in f:
        out["scp_src"] = dict({k: f[name] for name, k in _blob_scp_sections("scp_")}, hw=tuple(d["blob_scp_hw"]))
        if d.get("blob_scp_all"):
            out["scp_src"]["all"] = True
    if d.get("blob_scp_n"):
        out["scp_src"] = [{k: f[name] for name, k in _blob_scp_sections("scp%d_" % i)} for i in range(d["blob_scp_n"])]
    return out


class SlotRing:
    """Page-locked shared memory the loader workers write their sample blobs into (round 6).

    torch's DataLoader pins in a THREAD of the training process: per batch it unpickles the tensors (one authenticated socket round
    trip per shared-memory segment, Python under the GIL), allocates pinned memory and copies.  With the Swin blocks replayed as
    graphs the step's only host-bound stretch is the RoI heads behind the proposal sampler's device->host read, and every time that
    thread takes the GIL there the GPU waits: +1.9 ms per step measured (27.6 against 25.7 ms).  Here ONE region is allocated in shared
    memory before the workers fork and page-locked once (dgx_host_register); worker w owns slots [w * per_worker, (w + 1) * per_worker)
    and writes its k-th sample into slot k % per_worker; the training process receives (offset, bytes) and uploads straight from the
    slot (dgx_memcpy_h2d_async) -- no pin thread, no per-batch allocation, nothing but a few integers crosses the queue.
    Reuse is safe by the DataLoader's own bookkeeping: a worker holds at most `prefetch_factor` batches that the training process has
    not consumed, so with (prefetch_factor + 2) batches of slots a slot is rewritten no earlier than two further batches of that worker
    have been consumed -- 2 x num_workers steps after its upload was issued."""

    def __init__(self, num_workers, per_worker, slot_bytes):
        from .. import _lib as L
        self.num_workers, self.per_worker, self.slot_bytes = int(num_workers), int(per_worker), (int(slot_bytes) + 4095) // 4096 * 4096
        n = self.num_workers * self.per_worker * self.slot_bytes
        st = os.statvfs("/dev/shm") if os.path.isdir("/dev/shm") else None
        if st is not None and st.f_bavail * st.f_frsize < n + (1 << 30):
            raise MemoryError("SlotRing: /dev/shm has %.1f GB free, %.1f GB needed" % (st.f_bavail * st.f_frsize / 1e9, n / 1e9))
        self.buf = torch.empty(n, dtype=torch.uint8).share_memory_()
        L.check(L.lib().dgx_host_register(self.buf.data_ptr(), n), "dgx_host_register")
        self._registered, self._pid = True, os.getpid()

    def offset(self, worker, k):
        return (worker * self.per_worker + k % self.per_worker) * self.slot_bytes

    def close(self):
        if self.__dict__.get("_registered") and self.__dict__.get("_pid") == os.getpid():      # (never from a forked worker)
            from .. import _lib as L
            L.lib().dgx_host_unregister(self.buf.data_ptr())
            self._registered = False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _RingCollate:
    """collate_fn (runs in the WORKER): the samples' blobs into this worker's next slots; what is returned carries (offset, bytes)."""

    def __init__(self, ring):
        self.ring, self.k = ring, 0

    def __call__(self, batch):
        info = torch.utils.data.get_worker_info()
        if info is None or self.ring is None:
            return batch
        for d in batch:
            blob = d.get("blob")
            if blob is None or blob.numel() > self.ring.slot_bytes:      # an image with more ground truth than a slot holds: the ordinary way
                continue
            off, n = self.ring.offset(info.id, self.k), int(blob.numel())
            self.k += 1
            self.ring.buf[off:off + n].copy_(blob)
            d["blob"], d["blob_slot"] = None, (off, n)
        return batch


class _MapDataset(torch.utils.data.Dataset):
    def __init__(self, dicts, fn):
        self.dicts, self.fn = dicts, fn

    def __len__(self):
        return len(self.dicts)

    def __getitem__(self, i):
        return self.fn(self.dicts[i])


def _worker_init(worker_id, base_seed, in_worker=True, pool=None):
    seed = (base_seed + worker_id) % (2 ** 31)
    np.random.seed(seed)
    torch.manual_seed(seed)
    if pool is not None:          # the instance pool's own `random` (blend-mode draws); the process's global `random` stays as it is
        pool.seed(seed)
    if in_worker:
        torch.set_num_threads(1)      # 16 workers per GPU: one core each


def _tensors_of(obj):
    """Every device tensor reachable from one batched-input dict (image, Instances fields, lazily indexed masks)."""
    if torch.is_tensor(obj):
        yield obj
    elif isinstance(obj, dict):
        for v in obj.values():
            yield from _tensors_of(v)
    elif isinstance(obj, (list, tuple)):
        for v in obj:
            yield from _tensors_of(v)
    elif isinstance(obj, Instances):
        yield from _tensors_of(obj.get_fields())
    elif isinstance(obj, Boxes):
        yield obj.tensor
    elif isinstance(obj, BitMasks):
        yield obj._base
        if obj._index is not None:
            yield obj._index


class BatchAhead:
    """Host batches (lists of worker results, CPU tensors) -> device batches, prepared ONE BATCH AHEAD on a side HIP stream.

    The copy-paste compositor is the data-loading side of the step (the reference runs it in loader workers): it depends on
    nothing the optimizer produces.  So while step t trains, the batch of step t+1 is uploaded (pinned memory, asynchronous)
    and composited on `side`, and its one data-dependent shape (objects that end up fully covered are dropped: one
    device->host count per image) is read back from THAT stream instead of draining the training stream.  __next__ hands over
    batch t (the training stream waits for its event and takes ownership of the tensors) and then issues batch t+1 -- before the
    caller's forward: the host is ahead of the GPU at that point, whereas after the forward's device->host read every host
    microsecond is GPU idle time.  bench.py's timed step is this class fed with fixed host batches; train_net.py's is this class
    fed by the DataLoader."""

    def __init__(self, host_batches, finish, device):
        self.it, self.finish, self.device = iter(host_batches), finish, torch.device(device)
        self.side = torch.cuda.Stream(self.device) if self.device.type == "cuda" else None
        self.nxt, self.started = None, False
        self.wait_s = 0.0                   # seconds __next__ last spent blocked on the workers (the loop's real data_time)

    def _compose(self):
        import time
        t0 = time.perf_counter()
        try:
            host = next(self.it)
        except StopIteration:
            return None
        self.wait_s = time.perf_counter() - t0
        if self.side is None:
            return [self.finish(d, self.device) for d in host], None
        with torch.cuda.stream(self.side):
            batch = [self.finish(d, self.device) for d in host]
            ev = torch.cuda.Event()
            ev.record(self.side)
        return batch, ev

    def __iter__(self):
        return self

    def __next__(self):
        if not self.started:
            self.started, self.nxt = True, self._compose()
        cur = self.nxt
        if cur is None:
            raise StopIteration
        batch, ev = cur
        if ev is not None:
            cs = torch.cuda.current_stream(self.device)
            cs.wait_event(ev)                       # the training stream consumes the composited tensors ...
            for t in _tensors_of(batch):            # ... and owns them from here on (allocator stream bookkeeping)
                if t.is_cuda:
                    t.record_stream(cs)
        self.nxt = self._compose()
        return batch


# Intra-op CPU threads of the TRAINING process while a loader runs.  torch sizes its thread pool by the visible cores (128 on the
# 256-core MI355X host), but the process shares a cgroup CPU quota with its workers (16 CPUs on the box measured: /sys/fs/cgroup/cpu.max
# 1600000 100000): the pin thread's 12-30 MB copies fanned out over 128 OpenMP threads whose spin-waits burnt the quota, the kernel
# throttled the whole cgroup, and the training thread's host time per step DOUBLED (profiles/r06_loader_ab.txt: 57.0 ms/step with the
# default pool, 28.5 with 4 threads, same workers, same batches; 25.2 with the same batches and no loader running).  The training
# process has no CPU tensor work of its own besides those copies.  bench.py --loader-dev main_threads=N overrides (0 = leave alone).
DEVICE_RASTER_CROSSING_BYTES = 4 << 20      # ring-slot allowance for one sample's crossing lists with INPUT.DEVICE_RASTER


DEVICE_RESIZE_TABLE_BYTES = 1 << 20         # ring-slot allowance for one sample's resize job table and coefficient tables with INPUT.DEVICE_RESIZE


def ring_slot_bytes(size, self_copy_sources=0, device_raster=False, device_resize=False):
    """Bytes of one SlotRing slot at TRAIN_SIZE `size`: 48 planes (the image and ~45 dense masks), 48 more per self-copy source, and
    8 MB for the rest of the blob.  INPUT.DEVICE_RASTER: no mask planes travel -- the 3 image planes, the same 8 MB, and
    DEVICE_RASTER_CROSSING_BYTES for the crossing lists and their offsets (4 bytes per crossing: room for a million, where 12 polygons
    of 120 vertices across 800 px make 70 000) -- never more than the slot without the key, which a small TRAIN_SIZE would otherwise
    fall below; a sample beyond its slot takes the ordinary way, as any blob larger than its slot does.  INPUT.DEVICE_RESIZE: the
    decoded source travels in place of the image; it can be larger than TRAIN_SIZE^2 (a downscale), so the 3 planes stay as its
    allowance, and DEVICE_RESIZE_TABLE_BYTES is added for the tables (4 bytes x (2 + ksize) per window row and column: 2 x 1024 x 5
    words = 40 KB for an upscale to 1024^2, 2 x 100 x 23 for a 10x downscale, a few KB per pool patch) -- again never more than the
    slot without the keys; the patch sources (at most DEVICE_RESIZE_MAX_SRC_RATIO x `flat`) fall under the 8 MB."""
    dense = size * size * (48 + 48 * int(self_copy_sources)) + (8 << 20)
    slot = min(dense, size * size * 3 + (8 << 20) + DEVICE_RASTER_CROSSING_BYTES) if device_raster else dense
    if device_resize:
        slot = min(dense, slot + DEVICE_RESIZE_TABLE_BYTES)
    return slot
DEV = {"pin": "ring", "strategy": None, "main_threads": 4}      # pin: "ring" (SlotRing) | "loader" (the DataLoader's pin thread) | "none"


def build_detection_train_loader(cfg, per_gpu, device, seed):
    """DG/train_net.py:164-239 + D2/data/build.py:build_detection_train_loader: dataset dicts, sampler by
    DATALOADER.SAMPLER_TRAIN, the whole mapper (copy-paste preparation included) in DATALOADER.NUM_WORKERS worker processes, each
    sample written by its worker into a slot of a page-locked shared-memory ring (SlotRing; the DataLoader's pin thread when the ring
    cannot be had); the training process only uploads and runs the compositor kernel, one batch ahead on a side stream (BatchAhead)."""
    import functools
    from ..config.image_labels import check_loader_keys
    name = cfg.DATALOADER.SAMPLER_TRAIN
    check_loader_keys(cfg, per_gpu)
    batch_sizes = None          # MultiDatasetSampler: the per-source sizes of its grouped batches
    if name == "MultiDatasetSampler":
        from .samplers import GroupedBatchSampler, MultiDatasetSampler
        n_src = len(cfg.DATASETS.TRAIN)
        dicts = get_detection_dataset_dicts_with_source(cfg.DATASETS.TRAIN, filter_empty=cfg.DATALOADER.FILTER_EMPTY_ANNOTATIONS,
                                                        dataset_ann=cfg.DATALOADER.DATASET_ANN)
        sampler = MultiDatasetSampler(dicts, list(cfg.DATALOADER.DATASET_RATIO)[:n_src], list(cfg.DATALOADER.USE_RFS)[:n_src],
                                      list(cfg.DATALOADER.DATASET_ANN)[:n_src], cfg.DATALOADER.REPEAT_THRESHOLD, seed=seed)
        batch_sizes = [int(b) for b in list(cfg.DATALOADER.DATASET_BS)[:n_src]] if cfg.DATALOADER.USE_DIFF_BS_SIZE else [int(per_gpu)]
        sampler = GroupedBatchSampler(sampler, dicts, batch_sizes)
        per_gpu = max(batch_sizes)          # the slot ring is sized for the largest batch
    elif name == "TrainingSampler":
        dicts = get_detection_dataset_dicts(cfg.DATASETS.TRAIN, filter_empty=cfg.DATALOADER.FILTER_EMPTY_ANNOTATIONS)
        sampler = TrainingSampler(len(dicts), seed=seed)
    elif name == "RepeatFactorTrainingSampler":
        dicts = get_detection_dataset_dicts(cfg.DATASETS.TRAIN, filter_empty=cfg.DATALOADER.FILTER_EMPTY_ANNOTATIONS)
        rf = RepeatFactorTrainingSampler.repeat_factors_from_category_frequency(dicts, cfg.DATALOADER.REPEAT_THRESHOLD)
        sampler = RepeatFactorTrainingSampler(rf, seed=seed)
    else:
        raise ValueError("Unknown training sampler: {}".format(name))
    mapper = CopyPasteMapper(DatasetMapper(cfg, True), cfg)
    if mapper.device_raster and torch.device(device).type != "cuda":
        raise NotImplementedError("INPUT.DEVICE_RASTER with device '{}': the masks are filled by dgx_polygons_to_bitmask on the GPU; "
                                  "there is no host fill behind the key".format(device))
    if mapper.device_resize and torch.device(device).type != "cuda":
        raise NotImplementedError("INPUT.DEVICE_RESIZE with device '{}': the image is resized by dgx_resize_bilinear_u8 on the GPU; "
                                  "there is no host resize behind the key".format(device))
    mapper.set_dataset(dicts)
    rank_seed = seed * 1009 + comm.get_rank() * 131
    nw = cfg.DATALOADER.NUM_WORKERS
    on_gpu = torch.device(device).type == "cuda"
    if DEV["strategy"]:
        torch.multiprocessing.set_sharing_strategy(DEV["strategy"])
    if DEV["main_threads"] and on_gpu and nw > 0:
        torch.set_num_threads(min(torch.get_num_threads(), int(DEV["main_threads"])))
    pin_thread, ring = on_gpu and DEV["pin"] == "loader", None
    if on_gpu and nw > 0 and DEV["pin"] == "ring":
        # one slot holds an image with up to ~45 ground-truth masks at TRAIN_SIZE^2 (more: that sample takes the ordinary way)
        # with a self-copy method the sample also carries the source image (3 planes) and up to 99 selected source masks, each at most
        # TRAIN_SIZE^2: room for ~45 more planes (the mean of the draw over a 90-object image); beyond that, the ordinary way again
        # (INPUT.SCP_NUM_SRC sources: that many times the source's share)
        slot = ring_slot_bytes(int(cfg.INPUT.TRAIN_SIZE), 0 if mapper.self_prob is None else int(mapper.num_src), mapper.device_raster,
                               mapper.device_resize)
        try:
            ring = SlotRing(nw, (int(cfg.DATALOADER.PREFETCH_FACTOR) + 2) * per_gpu, slot)
        except Exception as e:
            logger.warning("loader: no page-locked slot ring (%s); falling back to the DataLoader's pin thread", e)
            pin_thread = True
    mapper.ring = ring
    how = dict(batch_sampler=sampler) if batch_sizes is not None else dict(sampler=sampler, batch_size=per_gpu, drop_last=True)
    loader = torch.utils.data.DataLoader(
        _MapDataset(dicts, mapper), num_workers=nw, **how,
        collate_fn=_RingCollate(ring) if ring is not None else _identity,
        worker_init_fn=functools.partial(_worker_init, base_seed=rank_seed, pool=mapper.inst_pool), pin_memory=pin_thread,
        prefetch_factor=cfg.DATALOADER.PREFETCH_FACTOR if nw > 0 else None, persistent_workers=nw > 0)
    if nw == 0:
        _worker_init(0, rank_seed, in_worker=False, pool=mapper.inst_pool)
    else:
        # The workers fork inside BatchAhead (iter(loader)).  Pinned host memory is not mapped into a forked child, so garbage of
        # this process that still holds pinned tensors is freed here, before the fork, and not by a worker's own collector.
        gc.collect()
    return BatchAhead(loader, mapper.finish, device)


def _identity(batch):
    return batch


def build_detection_test_loader(cfg, dataset_name, device):
    """D2/data/build.py:build_detection_test_loader: every image once, sharded over ranks by InferenceSampler, batch size 1,
    test-time mapper (no annotations)."""
    from .samplers import InferenceSampler
    dicts = get_detection_dataset_dicts([dataset_name], filter_empty=False)
    mapper = DatasetMapper(cfg, False)
    loader = torch.utils.data.DataLoader(_MapDataset(dicts, mapper), sampler=InferenceSampler(len(dicts)), batch_size=1,
                                         num_workers=cfg.DATALOADER.NUM_WORKERS, collate_fn=lambda b: b)
    for batch in loader:
        for d in batch:
            d["image"] = d["image"].to(device, non_blocking=True)
        yield batch
