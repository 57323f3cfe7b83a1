"""Multi-GPU layer: one process per GPU, instances sharded across ranks, ONE result gather.

The reference scales out only by running separate processes over contiguous index ranges
(``--start_index/--end_index/--gpu_idx``, reference src/batch_scripts/whole.py:25-27,42); instances
are independent, so the data path needs no collective.  The only exchange is the final gather of
the (n_i, 39) box tensors (+ status) to one rank — RCCL over xGMI on GPUs (torch.distributed backend
"nccl"), gloo on CPU in the tests.

Partitioning works on METADATA only (image index and an area per instance — the annotation's ``area`` field, or
``mask_stats_rle`` / ``mask_stats_poly``): no rank ever looks at another rank's masks, so a rank only has to hold
(or load) the depth planes and masks of its own contiguous image range (COCO-train: 264 GB of u8 masks in total,
33 GB per rank with 8 GPUs).
"""
from __future__ import annotations

from typing import Callable, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.distributed as dist

from .batched import fit_instances, refuse_depth16
from .masks import annotation_areas, fit_annotations_all


def partition_contiguous(costs: Sequence[float], world: int) -> List[Tuple[int, int]]:
    """Split items 0..n-1 into ``world`` contiguous [start, end) ranges with balanced total cost
    (cost of an image = sum of its instances' mask areas + one depth plane).  Contiguous ranges keep
    every image's instances — and its depth plane — on one GPU, like the reference's index ranges."""
    c = np.asarray(costs, dtype=np.float64)
    n = len(c)
    if world <= 0:
        raise ValueError("world must be positive")
    cum = np.concatenate([[0.0], np.cumsum(c)])
    total = cum[-1]
    cuts = [0]
    for r in range(1, world):
        target = total * r / world
        k = int(np.searchsorted(cum, target, side="left"))
        # choose the boundary whose prefix cost is closest to the target
        if k > 0 and (k > n or abs(cum[k - 1] - target) <= abs(cum[min(k, n)] - target)):
            k -= 1
        cuts.append(min(max(k, cuts[-1]), n))
    cuts.append(n)
    return [(cuts[i], cuts[i + 1]) for i in range(world)]


class Shard(NamedTuple):
    """One rank's share: images [img_lo, img_hi) and their instances [inst_lo, inst_hi) of the global lists."""
    img_lo: int
    img_hi: int
    inst_lo: int
    inst_hi: int


def plan_shards(image_index, num_images: int, world: int, areas=None, frame_pixels: int = 640 * 480) -> List[Shard]:
    """Cost-balanced contiguous image ranges from metadata only.

    image_index  (B,) non-decreasing image of every instance
    areas        (B,) mask area per instance in pixels (annotation ``area``, ``mask_stats_rle(...)[:, 0]``, ...) or None
                 (then every instance counts as one mean-size mask)
    Cost model of an image (what the fit kernel moves for it): one depth plane (4 B/px) if it has instances + per
    instance one mask plane (1 B/px) + its masked depth pixels twice (2 x 4 B x area)."""
    img = np.asarray(image_index.cpu() if isinstance(image_index, torch.Tensor) else image_index).astype(np.int64)
    if img.size and (np.diff(img) < 0).any():
        raise ValueError("image_index must be non-decreasing (instances grouped by image)")
    if img.size and (img.min() < 0 or img.max() >= num_images):
        raise ValueError("image_index out of range")
    hw = float(frame_pixels)
    if areas is None:
        a = np.full(img.shape, 0.1 * hw)
    else:
        a = np.asarray(areas.cpu() if isinstance(areas, torch.Tensor) else areas, dtype=np.float64)
        if a.shape != img.shape:
            raise ValueError("areas must have one entry per instance")
    per_inst = hw + 8.0 * a
    cost = np.bincount(img, weights=per_inst, minlength=num_images) + 4.0 * hw * (np.bincount(img, minlength=num_images) > 0)
    out = []
    for lo, hi in partition_contiguous(cost, world):
        ilo, ihi = int(np.searchsorted(img, lo, side="left")), int(np.searchsorted(img, hi, side="left"))
        out.append(Shard(lo, hi, ilo, ihi))
    return out


def _is_gloo(group) -> bool:
    try:
        return dist.get_backend(group) == "gloo"
    except Exception:  # noqa: BLE001
        return False


def gather_boxes(boxes: torch.Tensor, status: torch.Tensor, dst: int = 0, group=None, counts=None):
    """Gather every rank's (n_i, 39) float64 records and (n_i,) int32 status to ``dst`` in rank order.

    ONE payload collective: the status rides as a 40th float64 column of the records (int32 -> float64 is exact), padded to the
    largest shard, one ``dist.gather``.  Ranks may hold different n_i: the counts are exchanged first (one tiny all_gather and
    the host read of its result) unless the caller already knows them - ``counts`` (a sequence of world_size ints, the same
    on every rank; what ``plan_shards`` or a fixed batch size gives) skips that round trip.  Returns ``(boxes, status, counts)``
    on ``dst`` and ``None`` elsewhere.  ~320 B per box: 860k boxes over 8 GPUs is 34 MB per rank - irrelevant next to the
    compute, so the simplest correct collective is used.  With the gloo backend (CPU tests, two ranks on one GPU) device
    tensors are staged through the host.
    """
    world = dist.get_world_size(group)
    rank = dist.get_rank(group)
    if _is_gloo(group) and boxes.is_cuda:
        boxes, status = boxes.cpu(), status.cpu()
    if counts is None:
        n = torch.tensor([boxes.shape[0]], dtype=torch.int64, device=boxes.device)
        cl = [torch.zeros_like(n) for _ in range(world)]
        dist.all_gather(cl, n, group=group)
        counts = [int(c) for c in cl]
    else:
        counts = [int(c) for c in counts]
        if len(counts) != world or counts[rank] != boxes.shape[0]:
            raise ValueError("gather_boxes: counts must list every rank's row count (this rank's does not match its tensor)")
    nmax = max(counts)
    payload = boxes.new_zeros((nmax, boxes.shape[1] + 1))
    payload[:boxes.shape[0], :boxes.shape[1]] = boxes
    payload[:boxes.shape[0], boxes.shape[1]] = status.to(boxes.dtype)
    try:
        gp = [torch.empty_like(payload) for _ in range(world)] if rank == dst else None
        dist.gather(payload, gp, dst=dst, group=group)
    except (RuntimeError, NotImplementedError) as e:
        # ONLY a backend that has no gather at all: every rank collects, dst keeps.  Anything else (a failed RCCL call, a
        # mismatched shape) must surface - falling back would hide the error and double the traffic.
        msg = str(e).lower()
        if not (isinstance(e, NotImplementedError) or "not supported" in msg or "not implemented" in msg or
                "does not support" in msg or "no backend" in msg):
            raise
        gp = [torch.empty_like(payload) for _ in range(world)]
        dist.all_gather(gp, payload, group=group)
    if rank != dst:
        return None
    allp = torch.cat([g[:c] for g, c in zip(gp, counts)])
    return allp[:, :boxes.shape[1]].contiguous(), allp[:, boxes.shape[1]].to(status.dtype), counts


def _check_method(method) -> None:
    """The reference's error for an unknown yaw method (src/util_3dbox.py:151), raised before any collective or device work.
    (Spelled out here: this module must import on ranks that have no GPU library loaded.)"""
    if method not in ("pca", "convex_hull"):
        raise ValueError(f"Unknown method: {method}. Use 'pca' or 'convex_hull'")


def _method_kw(method) -> dict:
    return {} if method == "pca" else {"method": method}   # (an injected fit_fn without the keyword keeps working for "pca")


def fit_instances_sharded(depth, masks, K, image_index, ground=None, sample_idx=None, areas=None, dst: int = 0, group=None,
                          fit_fn: Optional[Callable] = None, load_fn: Optional[Callable] = None, timings: Optional[dict] = None,
                          method: str = "pca"):
    """Every rank passes the same METADATA (``image_index``, optionally ``areas``); images are split into contiguous,
    cost-balanced ranges (``plan_shards``), each rank fits the instances of its images on its own GPU and the records are
    gathered on ``dst`` in global instance order.

    Two ways to supply the tensors:
      * global tensors ``depth (P,H,W)``, ``masks (B,H,W)``, ``K (P,3,3) | (3,3)``, ``ground``, ``sample_idx``: only this
        rank's slices are ever indexed (views — nothing is computed over the global tensors);
      * ``load_fn(shard) -> (depth, masks, K, ground, sample_idx)`` returning ONLY this rank's images / instances (depth planes
        img_lo..img_hi, masks inst_lo..inst_hi); pass ``depth=(P, H, W)`` (the global shape) and ``masks=None``.
    ``areas`` (B,) are per-instance mask areas for the balance (None: count-based).  ``fit_fn`` defaults to
    labelany3d_amd.fit_instances (injectable so the sharding logic is testable on CPU with gloo).  ``timings`` (a dict, optional):
    filled with this rank's ``load_s`` / ``fit_s`` / ``gather_s`` wall-clock seconds (the device is synchronised around each
    stage then, which a production call has no reason to do) and its shard.  ``method``: "pca" | "convex_hull", handed to
    ``fit_fn`` as a keyword when it is not "pca"."""
    refuse_depth16(depth, "shard.fit_instances_sharded")
    _check_method(method)
    if fit_fn is None:
        fit_fn = fit_instances
    world = dist.get_world_size(group)
    rank = dist.get_rank(group)
    img = np.asarray(image_index.cpu() if isinstance(image_index, torch.Tensor) else image_index).astype(np.int64)
    if load_fn is not None:
        P, H, W = (int(v) for v in depth)
    else:
        P, H, W = depth.shape
    plan = plan_shards(img, P, world, areas=areas, frame_pixels=H * W)
    sh = plan[rank]
    local_img = (img[sh.inst_lo:sh.inst_hi] - sh.img_lo).astype(np.int32)
    import time

    def _sync():
        if timings is not None and torch.cuda.is_available():
            torch.cuda.synchronize()
        return time.perf_counter()
    t0 = _sync()
    if load_fn is not None:
        d, m, k, g, si = load_fn(sh)
    else:
        d = depth[sh.img_lo:sh.img_hi]
        m = masks[sh.inst_lo:sh.inst_hi]
        k = K
        if hasattr(K, "shape") and len(K.shape) == 3 and K.shape[0] == P:
            k = K[sh.img_lo:sh.img_hi]
        g = None if ground is None else ground[sh.inst_lo:sh.inst_hi]
        si = None if sample_idx is None else sample_idx[sh.inst_lo:sh.inst_hi]
    t1 = _sync()
    if sh.inst_hi > sh.inst_lo:
        boxes, status, _ = fit_fn(d, m, k, ground=g, sample_idx=si, image_index=local_img, **_method_kw(method))
    else:  # a rank without instances still takes part in the gather
        dev = m.device if isinstance(m, torch.Tensor) else torch.device("cpu")
        boxes = torch.zeros((0, 39), dtype=torch.float64, device=dev)
        status = torch.zeros((0,), dtype=torch.int32, device=dev)
    t2 = _sync()
    # every rank knows every shard's size from the plan: no count exchange
    out = gather_boxes(boxes, status, dst=dst, group=group, counts=[p.inst_hi - p.inst_lo for p in plan])
    if timings is not None:
        t3 = _sync()
        timings.update(load_s=t1 - t0, fit_s=t2 - t1, gather_s=t3 - t2, shard=tuple(sh), plan=[tuple(p) for p in plan])
    return out


def fit_annotations_sharded(annotations, image_size, image_index, num_images: int, depth_loader: Callable, ground=None, areas=None,
                            filter=None, dst: int = 0, group=None, fit_fn: Optional[Callable] = None, timings: Optional[dict] = None,
                            method: str = "pca"):
    """BASELINE config 4 on the reference's own annotation formats (round 5): COCO / COCONut annotations - polygon parts or run
    lengths, ``src/util.py:336-383``, ``src/download_coconut.py:167-199`` - sharded per image across the ranks, never expanded to
    u8 planes (860 k instances are 264 GB of planes and < 1 GB of polygons / run lengths; the fit kernel decodes them into its LDS
    bit image).  Every rank passes the SAME metadata - the annotation list (dicts with ``segmentation`` and, ideally, ``area``),
    the image of every annotation (non-decreasing, like the reference's per-image index ranges ``whole.py:25-27,42``) - and a
    ``depth_loader(shard) -> (depth (P_local, H, W) f32, K (3,3) | (P_local,3,3))`` that materialises ONLY the depth planes of images
    [shard.img_lo, shard.img_hi).  Plan: ``plan_shards`` on the annotations' ``area`` fields (``areas=`` overrides; None and no
    ``area`` fields: count-based).  Each rank fits its annotation range in one launch per segmentation kind
    (``masks.fit_annotations_all``; ``filter`` = the reference's keep rule fused into the fit) and the records travel to ``dst`` in ONE
    gather, one record per annotation in global order (status 6 = skipped / dropped by the keep rule).
    ``fit_fn(annotations, image_size, depth, K, ground=, image_index=, filter=) -> (boxes, status)`` is injectable (CPU tests).
    ``method``: "pca" | "convex_hull", handed to ``fit_fn`` as a keyword when it is not "pca"."""
    _check_method(method)
    if fit_fn is None:
        fit_fn = fit_annotations_all
    world = dist.get_world_size(group)
    rank = dist.get_rank(group)
    img = np.asarray(image_index.cpu() if isinstance(image_index, torch.Tensor) else image_index).astype(np.int64)
    if len(annotations) != img.shape[0]:
        raise ValueError("image_index must have one entry per annotation")
    if areas is None and len(annotations) and all("area" in a for a in annotations):
        areas = annotation_areas(annotations)
    W, H = int(image_size[0]), int(image_size[1])
    plan = plan_shards(img, num_images, world, areas=areas, frame_pixels=H * W)
    sh = plan[rank]
    import time

    def _sync():
        if timings is not None and torch.cuda.is_available():
            torch.cuda.synchronize()
        return time.perf_counter()
    t0 = _sync()
    depth, K = depth_loader(sh)
    refuse_depth16(depth, "shard.fit_annotations_sharded")
    t1 = _sync()
    n = sh.inst_hi - sh.inst_lo
    if n > 0:
        g = None if ground is None else ground[sh.inst_lo:sh.inst_hi]
        boxes, status = fit_fn(annotations[sh.inst_lo:sh.inst_hi], (W, H), depth, K, ground=g,
                               image_index=(img[sh.inst_lo:sh.inst_hi] - sh.img_lo).astype(np.int32), filter=filter, **_method_kw(method))
    else:  # a rank without annotations still takes part in the gather
        dev = depth.device if isinstance(depth, torch.Tensor) else torch.device("cpu")
        boxes = torch.zeros((0, 39), dtype=torch.float64, device=dev)
        status = torch.zeros((0,), dtype=torch.int32, device=dev)
    t2 = _sync()
    out = gather_boxes(boxes, status, dst=dst, group=group, counts=[p.inst_hi - p.inst_lo for p in plan])
    if timings is not None:
        t3 = _sync()
        timings.update(load_s=t1 - t0, fit_s=t2 - t1, gather_s=t3 - t2, shard=tuple(sh), plan=[tuple(p) for p in plan])
    return out
