"""Online pair source: rendered training pairs go straight into RAFT-layout batches on the GPU, nothing touches disk.

    src = OnlinePairs(base, batch_size=8, crop=(288, 960), mpi_from="model", ckpt_path="random:3")
    for batch in src:            # one epoch; dict(image1, image2 [B,3,h,w] RGB 0..255, flow [B,2,h,w], valid [B,h,w]) + batch["meta"]
        loss = train_step(batch["image1"], batch["image2"], batch["flow"], batch["valid"])

What a batch holds is what gen_3dphoto_dynamic.py would have written for the same seed and producer flags (same instance ids, poses,
renders and hole fill), then RAFT's FlowAugmentor.spatial_transform (resize, stretch, flips, crop; RAFT/core/utils/augmentor.py:67-109)
and its dataset's packing (RAFT/core/datasets.py:85-90), fused into one mpf_augment_pairs launch per batch.  photometric=True (or a dict of
RAFT_PHOTOMETRIC's keys) adds the photometric half in front of it, as FlowAugmentor.__call__ orders them: ColorJitter (symmetric or
asymmetric) and the eraser on the full-size u8 frames, bit for bit PIL's arithmetic given the draws (mpf_photometric_pairs); the batch then
carries batch["photo_meta"].  photometric=None (the default) leaves the batches exactly as they are without it.

Schedule contract (the CLI's, gen_3dphoto_dynamic.py main()): private random.Random(seed) / np.random.RandomState(seed) streams; per
image with at least one instance in its mask, `pairs_per_image` x (instance id from numpy, dynamic pose, camera pose from `random`);
images without one draw nothing and are skipped.  Every rank replays the whole schedule and renders the images i with i % world == rank.
Epoch e+1 continues both streams where epoch e stopped.  shuffle=True: the image order of every epoch is a permutation drawn from a
third private stream, and the schedule draws are consumed in that processing order.  A fourth private stream picks the samples of a
batch out of the shuffle buffer (`mix` pairs; 0 = first in, first out) and draws their augmentation parameters.  A fifth one draws the
photometric parameters, so the spatial draws (flow, valid, meta) are the same with photometric augmentation on or off.  sparse=True takes
RAFT's sparse path instead (SparseFlowAugmentor, its KITTI stage): KITTI's 16-bit flow code, the nearest-pixel flow resize that leaves holes
(valid = 0), h-flip only and the margin crop, in one mpf_augment_sparse_pairs launch; its draws use the same two streams.  The batches are a
pure function of the arguments - not of `prefetch`, the fill pool or timing - and state_dict() / load_state_dict() resume them exactly.

The source never touches the global `random`, `np.random` or torch RNGs, nor torch.set_num_threads.
"""
import collections
import os
import queue
import threading

import numpy as np
import torch
import torch.utils.data

from . import _lib, io_formats, ops, pipeline, producer
from .producer import Schedule, mpi_from_disparity  # noqa: F401 - online.Schedule / online.mpi_from_disparity
from .utils import utils as U

MASK_THRESH = pipeline.MASK_THRESH

# RAFT's FlowAugmentor photometric settings (augmentor.py:32-34, 52): ColorJitter(0.4, 0.4, 0.4, 0.5 / 3.14), asymmetric with probability
# 0.2, the eraser with probability 0.5 and rectangle extents randint(50, 100)
RAFT_PHOTOMETRIC = dict(brightness=0.4, contrast=0.4, saturation=0.4, hue=0.5 / 3.14, asymmetric_prob=0.2, eraser_prob=0.5, eraser_bounds=(50, 100))
# RAFT's SparseFlowAugmentor photometric settings (augmentor.py:131-158): ColorJitter(0.3, 0.3, 0.3, 0.3 / 3.14), always symmetric (its
# color_transform never draws the asymmetric case), the same eraser
RAFT_SPARSE_PHOTOMETRIC = dict(brightness=0.3, contrast=0.3, saturation=0.3, hue=0.3 / 3.14, asymmetric_prob=0.0, eraser_prob=0.5, eraser_bounds=(50, 100))
# RAFT's KITTI stage (core/datasets.py:374-378): the sparse augmentor with these settings
RAFT_KITTI_AUGMENT = dict(min_scale=-0.2, max_scale=0.4, do_flip=False)
SPARSE_AUGMENT_KEYS = ("min_scale", "max_scale", "do_flip", "spatial_aug_prob")     # what SparseFlowAugmentor.spatial_transform reads


def default_fill_threads():
    """The CPUs this process may run on minus 4 (the producer thread, the decoders, the trainer's own thread), clamped to 2..32."""
    try:
        cores = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        cores = os.cpu_count() or 8
    return max(2, min(32, cores - 4))


# ---- host side: the augmentation draws (no GPU) -------------------------------------------------------------------------------

def augment_params(rs, H, W, crop, augment):
    """One sample's parameters by RAFT's FlowAugmentor.spatial_transform rules (augmentor.py:67-109), drawn from the RandomState `rs`:
    min_scale clip max((h+8)/H, (w+8)/W); scale = 2**U(min_scale, max_scale); stretch with probability 0.8 (2**U(-0.2, 0.2) per axis);
    resize with probability 0.8 (cv2's size: rint(W * scale_x), rint(H * scale_y)); h-flip 0.5 and v-flip 0.1 when do_flip;
    y0 = randint(0, Hr - h), x0 = randint(0, Wr - w) (0 without a draw when equal).  augment=None: no resize, no flips, crop only."""
    h, w = crop
    p = dict(resize=0, scale_x=1.0, scale_y=1.0, Hr=H, Wr=W, flip_h=0, flip_v=0, y0=0, x0=0)
    if augment is not None:
        a = dict(min_scale=-0.2, max_scale=0.5, do_flip=True, stretch_prob=0.8, max_stretch=0.2, spatial_aug_prob=0.8, h_flip_prob=0.5, v_flip_prob=0.1)
        a.update(augment)
        min_scale = np.maximum((h + 8) / float(H), (w + 8) / float(W))
        scale = 2 ** rs.uniform(a["min_scale"], a["max_scale"])
        scale_x = scale_y = scale
        if rs.rand() < a["stretch_prob"]:
            scale_x *= 2 ** rs.uniform(-a["max_stretch"], a["max_stretch"])
            scale_y *= 2 ** rs.uniform(-a["max_stretch"], a["max_stretch"])
        scale_x = float(np.clip(scale_x, min_scale, None))
        scale_y = float(np.clip(scale_y, min_scale, None))
        if rs.rand() < a["spatial_aug_prob"]:
            p.update(resize=1, scale_x=scale_x, scale_y=scale_y, Hr=int(np.rint(H * scale_y)), Wr=int(np.rint(W * scale_x)))
        if a["do_flip"]:
            if rs.rand() < a["h_flip_prob"]:
                p["flip_h"] = 1
            if rs.rand() < a["v_flip_prob"]:
                p["flip_v"] = 1
    if p["Hr"] < h or p["Wr"] < w:
        raise ValueError("crop %s does not fit the %d x %d frame" % (crop, p["Hr"], p["Wr"]))
    p["y0"] = int(rs.randint(0, p["Hr"] - h)) if p["Hr"] > h else 0
    p["x0"] = int(rs.randint(0, p["Wr"] - w)) if p["Wr"] > w else 0
    return p


def sparse_augment_params(rs, H, W, crop, augment):
    """One sample's parameters by RAFT's SparseFlowAugmentor.spatial_transform rules and order (augmentor.py:194-232), drawn from the
    RandomState `rs`: s = clip(2**U(min_scale, max_scale), max((h+1)/H, (w+1)/W)) in float64, one scale for both axes; resize with probability
    spatial_aug_prob (size rint(H*s) x rint(W*s)); h-flip with probability 0.5 when do_flip (no v-flip); y0 = randint(0, Hr-h+20) and
    x0 = randint(-50, Wr-w+50), always drawn, then clipped to the frame.  augment=None: no resize, no flip, the crop drawn by the same margin
    rule.  -> the sample dict of ops.augment_sparse_pairs (without the pointers and quantize)."""
    h, w = crop
    p = dict(resize=0, scale_x=1.0, scale_y=1.0, Hr=H, Wr=W, flip_h=0, y0=0, x0=0)
    if augment is not None:
        a = dict(min_scale=-0.2, max_scale=0.5, do_flip=False, spatial_aug_prob=0.8)
        a.update(augment)
        min_scale = np.maximum((h + 1) / float(H), (w + 1) / float(W))
        scale = float(np.clip(2 ** rs.uniform(a["min_scale"], a["max_scale"]), min_scale, None))
        if rs.rand() < a["spatial_aug_prob"]:
            p.update(resize=1, scale_x=scale, scale_y=scale, Hr=int(np.rint(H * scale)), Wr=int(np.rint(W * scale)))
        if a["do_flip"] and rs.rand() < 0.5:
            p["flip_h"] = 1
    if p["Hr"] < h or p["Wr"] < w:
        raise ValueError("crop %s does not fit the %d x %d frame" % (crop, p["Hr"], p["Wr"]))
    y0 = int(rs.randint(0, p["Hr"] - h + 20))
    x0 = int(rs.randint(-50, p["Wr"] - w + 50))
    p["y0"], p["x0"] = min(max(y0, 0), p["Hr"] - h), min(max(x0, 0), p["Wr"] - w)
    return p


def sparse_config(sparse, augment):
    """sparse= (and augment=) of OnlinePairs -> dict(quantize) or None (the dense path); checks that augment holds only the keys
    SparseFlowAugmentor reads (it has no stretch and no v-flip)."""
    if sparse is None or sparse is False:
        return None
    c = dict(quantize=True)
    if sparse is not True:
        unknown = set(sparse) - set(c)
        if unknown:
            raise ValueError("sparse: unknown keys %s" % sorted(unknown))
        c.update(sparse)
    c["quantize"] = bool(c["quantize"])
    if augment is not None:
        unknown = set(augment) - set(SPARSE_AUGMENT_KEYS)
        if unknown:
            raise ValueError("sparse augmentation reads only %s, not %s" % (", ".join(SPARSE_AUGMENT_KEYS), sorted(unknown)))
    return c


def photometric_config(photometric, sparse=False):
    """photometric= of OnlinePairs -> a complete, checked settings dict (None stays None; True = RAFT_PHOTOMETRIC, or RAFT_SPARSE_PHOTOMETRIC
    with sparse, which also refuses an asymmetric_prob > 0)."""
    if photometric is None or photometric is False:
        return None
    c = dict(RAFT_SPARSE_PHOTOMETRIC if sparse else RAFT_PHOTOMETRIC)
    if photometric is not True:
        unknown = set(photometric) - set(c)
        if unknown:
            raise ValueError("photometric: unknown keys %s" % sorted(unknown))
        c.update(photometric)
    for k in ("brightness", "contrast", "saturation"):
        c[k] = float(c[k])
        if not 0 <= c[k] < float("inf"):
            raise ValueError("photometric: %s must be a finite value >= 0" % k)
    c["hue"] = float(c["hue"])
    if not 0 <= c["hue"] <= 0.5:
        raise ValueError("photometric: hue must be in [0, 0.5]")
    for k in ("asymmetric_prob", "eraser_prob"):
        c[k] = float(c[k])
        if not 0 <= c[k] <= 1:
            raise ValueError("photometric: %s must be a probability" % k)
    lo, hi = (int(v) for v in c["eraser_bounds"])
    if not 1 <= lo < hi:
        raise ValueError("photometric: eraser_bounds must be (lo, hi) with 1 <= lo < hi")
    c["eraser_bounds"] = (lo, hi)
    if sparse and c["asymmetric_prob"] > 0:
        raise ValueError("photometric: the sparse augmentor's colour jitter is always symmetric (asymmetric_prob must be 0)")
    return c


def jitter_params(rs, c):
    """One ColorJitter parameter set by torchvision's get_params rules, drawn from the RandomState `rs`: permutation(4), then
    uniform(max(0, 1 - v), 1 + v) for brightness, contrast and saturation and uniform(-hue, hue), each rounded to float32 (torchvision draws
    them as float tensors); a setting of 0 is neither drawn nor applied.  -> dict(order (op codes of ops.PHOTO_OPS), brightness, contrast,
    saturation, hue, hue_shift = int(hue * 255.0)); factors of skipped ops are 1."""
    perm = [int(v) for v in rs.permutation(4)]
    p = dict(brightness=1.0, contrast=1.0, saturation=1.0, hue=0.0, hue_shift=0)
    for k in ("brightness", "contrast", "saturation"):
        if c[k] > 0:
            p[k] = float(np.float32(rs.uniform(max(0.0, 1.0 - c[k]), 1.0 + c[k])))
    if c["hue"] > 0:
        p["hue"] = float(np.float32(rs.uniform(-c["hue"], c["hue"])))
        p["hue_shift"] = int(p["hue"] * 255.0)
    p["order"] = [o for o in perm if c[ops.PHOTO_OPS[o]] > 0]
    return p


def photometric_params(rs, H, W, c, asymmetric=True):
    """One sample's photometric draws in RAFT's order (augmentor.py:36-65): asymmetric = rand() < asymmetric_prob, one jitter parameter set
    (two when asymmetric: image 1's, then image 2's), then the eraser: rand() < eraser_prob, randint(1, 3) rectangles of randint(0, W),
    randint(0, H), randint(*bounds) x 2 (x0, y0, dx, dy).  asymmetric=False (SparseFlowAugmentor, augmentor.py:135-158): no asymmetric draw,
    always symmetric.  -> dict(joint, jitter, rects), the sample format of ops.photometric_pairs."""
    asym = asymmetric and rs.rand() < c["asymmetric_prob"]
    jitter = [jitter_params(rs, c) for _ in range(2 if asym else 1)]
    rects = []
    if rs.rand() < c["eraser_prob"]:
        for _ in range(int(rs.randint(1, 3))):
            x0, y0 = int(rs.randint(0, W)), int(rs.randint(0, H))
            dx, dy = int(rs.randint(*c["eraser_bounds"])), int(rs.randint(*c["eraser_bounds"]))
            rects.append((x0, y0, dx, dy))
    return dict(joint=0 if asym else 1, jitter=jitter, rects=rects)


class _Stop(Exception):
    pass


class OnlinePairs:
    """Iterable source of augmented training batches rendered on the GPU (module docstring).  Iterating yields one epoch.

    base: the CLI's input layout (base/{images,disps,masks}[, mpis]).  crop: (h, w), None = the full frame.  mpi_from: model | npz | disparity;
    ckpt_path: checkpoint or "random:SEED" (model); model_dtype: auto | fp16 (HipPredictor, graph) or fp32 | fp32-mfma | fp64 (PrecisePredictor).
    fill: auto | builtin | ns-hip | peel | none (the CLI's --inpaint; cv2 where installed).  ns-hip: builtin's NS fill on the GPU, the same bytes
    as builtin without the host threads (one batched call per image's pairs on the tail stream); parity with cv2 itself is unpinned, as for builtin.  augment: dict of RAFT's FlowAugmentor settings, None = none.
    photometric: None = none, True = RAFT_PHOTOMETRIC, or a dict of its keys (the rest from RAFT_PHOTOMETRIC).
    sparse: None = RAFT's dense FlowAugmentor path; True or dict(quantize=True) = its sparse path (SparseFlowAugmentor, the KITTI stage): the
    flow through KITTI's 16-bit code (quantize), nearest-pixel flow resize with holes, h-flip only, margin crop; augment= then takes only
    SPARSE_AUGMENT_KEYS (RAFT_KITTI_AUGMENT is the KITTI stage's), and photometric=True means RAFT_SPARSE_PHOTOMETRIC.
    mix: shuffle-buffer size in pairs (0 = off).  prefetch: batches enqueued ahead of the consumer.  rank / world_size: default from
    torch.distributed or RANK / WORLD_SIZE.  fill_threads: host threads of fill="builtin" (default: default_fill_threads()).
    disp_filter: None = none, or the windows of the sparse bilateral filter, such as (5, 5), run on every disparity before the input stage
    (the CLI's --disp-filter).  adjust_planes: False = the fixed planes; True = the checkpoint's plane-adjustment network moves them per image (the
    CLI's --adjust-planes; mpi_from="model" only); an image for which it puts a plane at a disparity of 0 or below is skipped (`skipped`)."""

    def __init__(self, base, batch_size=8, crop=(288, 960), width=1280, height=384, seed=114514, ext_cz=0.15, pairs_per_image=5, poses="v2",
                 mpi_from="model", ckpt_path=None, model_dtype="auto", fill="auto", augment=dict(min_scale=-0.2, max_scale=0.5, do_flip=True),
                 shuffle=True, mix=32, prefetch=2, rank=None, world_size=None, device=None, planes=64, fill_threads=None, photometric=None,
                 sparse=None, disp_filter=None, adjust_planes=False):
        if torch.utils.data.get_worker_info() is not None:
            raise RuntimeError("OnlinePairs renders on the GPU in the training process: construct it there, not inside a DataLoader worker")
        if mpi_from not in ("model", "npz", "disparity"):
            raise ValueError("mpi_from must be model, npz or disparity")
        if batch_size < 1 or pairs_per_image < 1 or mix < 0 or prefetch < 0:
            raise ValueError("batch_size and pairs_per_image must be >= 1, mix and prefetch >= 0")
        self.base, self.B, self.W, self.H = base, int(batch_size), int(width), int(height)
        self.crop = (self.H, self.W) if crop is None else (int(crop[0]), int(crop[1]))
        if self.crop[0] > self.H or self.crop[1] > self.W:
            raise ValueError("crop %s is larger than the %d x %d frame" % (self.crop, self.H, self.W))
        self.seed, self.ext_cz, self.R, self.poses = int(seed), float(ext_cz), int(pairs_per_image), poses
        self.mpi_from, self.augment, self.shuffle, self.mix, self.prefetch = mpi_from, (None if augment is None else dict(augment)), shuffle, int(mix), int(prefetch)
        self.sparse = sparse_config(sparse, self.augment)
        self.photometric = photometric_config(photometric, sparse=self.sparse is not None)
        self.disp_filter = producer.parse_disp_filter(disp_filter)
        self.adjust_planes = bool(adjust_planes)
        if self.adjust_planes and mpi_from != "model":
            raise ValueError("adjust_planes runs the checkpoint's plane-adjustment network: it goes with mpi_from='model'")
        if rank is None or world_size is None:
            import torch.distributed as dist
            if dist.is_available() and dist.is_initialized():
                r, w = dist.get_rank(), dist.get_world_size()
            else:
                r, w = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
            rank = r if rank is None else rank
            world_size = w if world_size is None else world_size
        if not 0 <= rank < world_size:
            raise ValueError("rank %d outside world %d" % (rank, world_size))
        self.rank, self.world = int(rank), int(world_size)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if self.device.type != "cuda":
            raise _lib.MpiFlowHipError("OnlinePairs renders with the HIP kernels of mpiflow_amd: device must be a GPU")
        _lib.load()
        fm = U.resolve_inpaint(fill)
        if fm not in ("cv2", "builtin", "ns-hip", "peel", "none"):
            raise ValueError("fill must be auto, builtin, ns-hip, peel or none")
        self.fill = fm
        self.fill_threads = int(fill_threads) if fill_threads else default_fill_threads()

        self.img_dir, self.disp_dir, self.mask_dir = (os.path.join(base, d) for d in ("images", "disps", "masks"))
        self.names = sorted(os.listdir(self.img_dir))
        self.mask_max = self._mask_table()
        self.skipped = []
        self._skipped_names = set()

        # the four (five with photometric augmentation) private streams and the position: everything state_dict() captures
        self._sched = Schedule(self.seed, self.ext_cz, self.R, poses)
        self._order_rs = np.random.RandomState([self.seed & 0xFFFFFFFF, 2])
        self._aug_rs = np.random.RandomState([self.seed & 0xFFFFFFFF, 1])
        self._photo_rs = np.random.RandomState([self.seed & 0xFFFFFFFF, 3]) if self.photometric is not None else None
        self._epoch, self._pos, self._order, self._batches = 0, 0, None, 0
        self._buf = []                    # shuffle buffer: dicts(job, r, src, dst, flow, wait)
        self._pending = []                # the pairs of the image rendered last: they join the buffer when the next image has been enqueued
        self._resume_buf = []             # (job, r) to re-render before anything else (load_state_dict): the buffer, then the pending pairs
        self._resume_pending = 0

        self._set_up_gpu(ckpt_path, model_dtype, planes)
        self._producer = None
        self._q = None
        self._stop = threading.Event()
        self._delivered = self._snapshot()
        self._closed = False

    # ---- set-up ------------------------------------------------------------------------------------------------------------------
    def _mask_table(self):
        import concurrent.futures
        import torch.distributed as dist
        if self.world > 1 and dist.is_available() and dist.is_initialized() and dist.get_world_size() == self.world:
            return pipeline.mask_max_table(self.names, self.mask_dir, self.rank, self.world)
        with concurrent.futures.ThreadPoolExecutor(max_workers=8) as pool:
            return list(pool.map(lambda nm: io_formats.mask_max_of_file(os.path.join(self.mask_dir, nm)), self.names))

    def _set_up_gpu(self, ckpt_path, model_dtype, planes):
        dev = self.device
        self.planes, model = int(planes), None
        with torch.cuda.device(dev):
            # created in this order, before the network's own streams: the order decides which of them share a hardware queue, and
            # creating the upload stream last cost the second and later sources of a process 30 % of their rate (tools/bench_online.py)
            self.stream = torch.cuda.Stream(device=dev)              # rendering, fill on the device, augmentation
            self.upload_stream = torch.cuda.Stream(device=dev)       # filled frames of fill="builtin" back to the device
            self.tail = torch.cuda.Stream(device=dev)                # hole fill (peel, ns-hip) / copies of the frames to the host (builtin)
            if self.mpi_from == "model":
                if ckpt_path is None:
                    raise ValueError("mpi_from='model' needs ckpt_path (a checkpoint, or random:SEED)")
                self.stream.wait_stream(torch.cuda.current_stream(dev))
                with torch.cuda.stream(self.stream):
                    model = producer.load_model(ckpt_path, self.W, self.H, self.planes, dev, adjust_planes=self.adjust_planes)
                self.planes = model.num_planes
            self.lane = producer.Lane(dev, self.H, self.W, self.planes, model, model_dtype, streams=(self.stream, self.tail), disp_filter=self.disp_filter)
            if model is not None and model_dtype in ("auto", "fp16"):
                # capture the network's graph here, on the constructing thread, not in the producer while other threads use the device
                with torch.cuda.stream(self.stream):
                    self.lane.predictor(torch.zeros((1, 3, self.H, self.W), device=dev), torch.full((1, 1, self.H, self.W), 0.5, device=dev))
        self._pool = None
        self._slots = []
        if self.fill in ("cv2", "builtin"):
            import concurrent.futures
            self._pool = concurrent.futures.ThreadPoolExecutor(max_workers=self.fill_threads, thread_name_prefix="online-fill")
            self._free_slots = collections.deque()
            self._busy_slots = collections.deque()               # (slot, upload event) in submission order
            self._n_slots = 2 * self.fill_threads + 2
        self.stream.synchronize()

    # ---- state -------------------------------------------------------------------------------------------------------------------
    def _snapshot(self):
        snap = dict(epoch=self._epoch, pos=self._pos, order=None if self._order is None else list(self._order), batches=self._batches,
                    sched=self._sched.state(), order_rs=self._order_rs.get_state(), aug_rs=self._aug_rs.get_state(),
                    buffer=[(e["job"], e["r"]) for e in self._buf + self._pending] if not self._resume_buf else list(self._resume_buf),
                    pending=len(self._pending) if not self._resume_buf else self._resume_pending)
        if self._photo_rs is not None:
            snap["photo_rs"] = self._photo_rs.get_state()
        return snap

    def state_dict(self):
        """The position after the last batch (or epoch end) handed to the consumer: epoch, image position, all four streams (+ photo_rs, the
        fifth, with photometric augmentation) and the identities of the pairs waiting in the shuffle buffer (re-rendered on resume)."""
        import copy
        return copy.deepcopy(self._delivered)

    def load_state_dict(self, st):
        import copy
        if self._photo_rs is not None and "photo_rs" not in st:
            raise ValueError("load_state_dict: this source augments photometrically, the state holds no photo_rs (saved without photometric=)")
        self._stop_producer()
        st = copy.deepcopy(st)
        self._epoch, self._pos, self._order, self._batches = st["epoch"], st["pos"], st["order"], st["batches"]
        self._sched.set_state(st["sched"])
        self._order_rs.set_state(st["order_rs"])
        self._aug_rs.set_state(st["aug_rs"])
        if self._photo_rs is not None:
            self._photo_rs.set_state(st["photo_rs"])
        self._buf, self._pending = [], []
        self._resume_buf = [(dict(job), r) for job, r in st["buffer"]]
        self._resume_pending = st["pending"]
        self._delivered = self._snapshot()

    # ---- iteration ---------------------------------------------------------------------------------------------------------------
    def __iter__(self):
        if self._closed:
            raise RuntimeError("OnlinePairs is closed")
        if self._producer is None:
            self._q = queue.Queue(maxsize=max(1, self.prefetch))
            self._stop.clear()
            self._producer = threading.Thread(target=self._produce, name="online-pairs", daemon=True)
            self._producer.start()
        while True:
            kind, payload, snap = self._q.get()
            if kind == "error":
                self._producer.join()
                self._producer = None
                raise payload
            self._delivered = snap
            if kind == "end":
                return
            yield self._hand_over(payload)

    def _hand_over(self, item):
        batch, ready = item
        cur = torch.cuda.current_stream(self.device)
        cur.wait_event(ready)
        for k in ("image1", "image2", "flow", "valid"):
            batch[k].record_stream(cur)
        return batch

    def _put(self, kind, payload):
        snap = self._snapshot()
        while True:
            if self._stop.is_set():
                raise _Stop()
            try:
                self._q.put((kind, payload, snap), timeout=0.1)
                return
            except queue.Full:
                continue

    def _produce(self):
        try:
            with torch.cuda.device(self.device), torch.no_grad():
                self._run()
        except _Stop:
            pass
        except BaseException as e:                                         # noqa: BLE001 - handed to the consumer
            try:
                self._q.put(("error", e, None), timeout=5)
            except queue.Full:
                pass

    def _run(self):
        cap = max(self.mix, self.B)
        if self._resume_buf:
            jobs = collections.OrderedDict()
            for job, r in self._resume_buf:
                jobs.setdefault(job["i"], (job, []))[1].append(r)
            rendered = {}
            items = iter(io_formats.InputPrefetcher(self.names, self.img_dir, self.disp_dir, self.mask_dir, list(jobs)))
            for i, (job, rs) in jobs.items():
                item = next(items)
                rendered[i] = {e["r"]: e for e in self._render(job, item, rs)}
            entries = [rendered[job["i"]][r] for job, r in self._resume_buf]
            cut = len(entries) - self._resume_pending
            self._buf, self._pending = entries[:cut], entries[cut:]
            self._resume_buf, self._resume_pending = [], 0
        while True:
            n = len(self.names)
            if self._order is None:
                self._order = [int(v) for v in self._order_rs.permutation(n)] if self.shuffle else list(range(n))
            owned = [i for i in self._order[self._pos:] if i % self.world == self.rank and self.mask_max[i] > 0]
            items = iter(io_formats.InputPrefetcher(self.names, self.img_dir, self.disp_dir, self.mask_dir, owned))
            while self._pos < n:
                i = self._order[self._pos]
                self._pos += 1
                name = self.names[i].split(".")[0]
                drawn = self._sched.draw(self.mask_max[i])
                if drawn is None:
                    if i % self.world == self.rank:
                        self._skip(name, "mask unreadable" if self.mask_max[i] < 0 else "mask holds no instance")
                    continue
                if i % self.world != self.rank:
                    continue
                item = next(items)
                assert item["i"] == i
                if item["error"] is not None:
                    self._skip(name, "input: %r" % (item["error"],))
                    continue
                job = dict(i=i, name=name, obj_indices=drawn[0], pose_params=drawn[1])
                try:
                    fresh = self._render(job, item, range(self.R))
                except _Stop:
                    raise
                except Exception as e:                                     # noqa: BLE001 - isolate the image, as the CLI does
                    self.stream.synchronize()
                    self._skip(name, "render: %r" % (e,))
                    continue
                # batches draw from the pairs of the images BEFORE this one: their host fills ran while this image was enqueued, so forming a
                # batch rarely waits for one, and the GPU already has this image's work (deterministic: the lag is one image, not a time)
                self._buf += self._pending
                self._pending = fresh
                while len(self._buf) >= cap:
                    self._put("batch", self._batch())
            self._buf += self._pending
            self._pending = []
            while len(self._buf) >= self.B:
                self._put("batch", self._batch())
            self._epoch, self._pos, self._order = self._epoch + 1, 0, None
            self._put("end", None)

    def _skip(self, name, why):
        if name not in self._skipped_names:
            self._skipped_names.add(name)
            self.skipped.append((name, why))

    # ---- rendering -----------------------------------------------------------------------------------------------------------------
    def _render(self, job, item, keep):
        """One image: the lane's front end (upload, input stage, MPI producer + blend), its pairs, hole fill.  -> buffer entries for the pairs
        r in `keep`."""
        keep = list(keep)
        with torch.cuda.stream(self.stream):
            front = self.lane.front(item, npz=os.path.join(self.base, "mpis", job["name"] + ".npz") if self.mpi_from == "npz" else None)
            src = self.lane.renderer.src_u8.clone()                      # the renderer's buffer is the next image's
            results = self.lane.pairs(front, job["obj_indices"], job["pose_params"])
            rendered = torch.cuda.Event()
            rendered.record(self.stream)
            dsts = [torch.empty((self.H, self.W, 3), dtype=torch.uint8, device=self.device) for _ in keep] if self.fill == "peel" else None
            if self.fill == "ns-hip" and keep:
                dsts = torch.empty((len(keep), self.H, self.W, 3), dtype=torch.uint8, device=self.device)
        # the fills run on a second stream, as the CLI's tail stream: the one-workgroup peel kernels / the copies to the host overlap the next
        # image's network instead of running in front of it.  Everything they read or write was allocated on self.stream and stays referenced
        # by the buffer entry until the batch that consumes it has been enqueued behind them (mpf_augment_pairs waits for `filled`).
        self.tail.wait_event(rendered)
        out = []
        with torch.cuda.stream(self.tail):
            if self.fill == "ns-hip" and keep:                           # the image's pairs in one call: one serial front per hole cluster
                frames = torch.stack([results[r]["frame_mix"] for r in keep])
                holes = torch.stack([results[r]["fill_mask"] for r in keep])
                ops.inpaint_ns(frames, holes, 3, out=dsts, workspace=self.lane.ns_workspace(len(keep)))
            for n, r in enumerate(keep):
                res = results[r]
                e = dict(job=job, r=r, src=src, flow=res["flow_mix"], wait=None, keep=res["slab"])
                if self.fill == "peel":
                    e["dst"] = ops.fill_holes(res["frame_mix"], res["fill_mask"], out=dsts[n], workspace=self.lane.fill_ws)
                elif self.fill == "ns-hip":
                    e["dst"] = dsts[n]
                elif self.fill == "none":
                    e["dst"] = res["frame_mix"]
                else:
                    e["dst"], e["wait"] = self._host_fill(res["frame_mix"], res["fill_mask"])
                out.append(e)
            if self.fill in ("peel", "ns-hip", "none"):
                filled = torch.cuda.Event()
                filled.record(self.tail)
                for e in out:
                    e["wait"] = filled
        return out

    def _slot(self):
        if self._free_slots:
            return self._free_slots.popleft()
        if len(self._free_slots) + len(self._busy_slots) < self._n_slots:
            pin = lambda *shape: torch.empty(shape, dtype=torch.uint8).pin_memory()    # noqa: E731
            return dict(frame=pin(self.H, self.W, 3), hole=pin(self.H, self.W), out=pin(self.H, self.W, 3))
        slot, fut = self._busy_slots.popleft()                            # the oldest: reused only after its upload has completed
        fut.result().synchronize()
        return slot

    def _host_fill(self, frame_mix, fill_mask):
        """fill="builtin" | "cv2": frame + hole mask to a pinned slot (on the render stream), fill on a pool thread, upload on the upload
        stream.  -> (device frame, future of the upload's event)."""
        while self._busy_slots and self._busy_slots[0][1].done() and self._busy_slots[0][1].result().query():
            self._free_slots.append(self._busy_slots.popleft()[0])
        slot = self._slot()
        slot["frame"].copy_(frame_mix, non_blocking=True)
        slot["hole"].copy_(fill_mask, non_blocking=True)
        copied = torch.cuda.Event()
        copied.record(torch.cuda.current_stream())
        with torch.cuda.stream(self.stream):                             # allocated where it is consumed
            dst = torch.empty((self.H, self.W, 3), dtype=torch.uint8, device=self.device)
        fill, dev, up = self.fill, self.device, self.upload_stream

        def work():
            copied.synchronize()
            if fill == "cv2":
                import cv2
                slot["out"].numpy()[...] = cv2.inpaint(slot["frame"].numpy(), slot["hole"].numpy(), 3, cv2.INPAINT_NS)
            else:
                ops.inpaint_host(slot["frame"].numpy(), slot["hole"].numpy(), 3, ops.INPAINT_NS, out=slot["out"].numpy())
            with torch.cuda.device(dev), torch.cuda.stream(up):
                dst.copy_(slot["out"], non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(up)
            return ev
        fut = self._pool.submit(work)
        self._busy_slots.append((slot, fut))
        return dst, fut

    # ---- batches -------------------------------------------------------------------------------------------------------------------
    def _batch(self):
        """B entries out of the buffer (uniformly from the augmentation stream when mixing, first in first out otherwise), their augmentation
        parameters, [one mpf_photometric_pairs launch into scratch frames,] one mpf_augment_pairs (mpf_augment_sparse_pairs with sparse=) launch.
        -> (batch dict, ready event)."""
        if self.mix > 0:
            picks = [int(v) for v in self._aug_rs.choice(len(self._buf), self.B, replace=False)]
            taken = [self._buf[j] for j in picks]
            gone = set(picks)
            self._buf = [e for j, e in enumerate(self._buf) if j not in gone]
        else:
            taken, self._buf = self._buf[:self.B], self._buf[self.B:]
        if self.sparse is None:
            params = [augment_params(self._aug_rs, self.H, self.W, self.crop, self.augment) for _ in taken]
        else:
            params = [sparse_augment_params(self._aug_rs, self.H, self.W, self.crop, self.augment) for _ in taken]
        photo = None if self._photo_rs is None else [photometric_params(self._photo_rs, self.H, self.W, self.photometric, asymmetric=self.sparse is None)
                                                     for _ in taken]
        with torch.cuda.stream(self.stream):
            for e in taken:
                if e["wait"] is not None:
                    self.stream.wait_event(e["wait"] if isinstance(e["wait"], torch.cuda.Event) else e["wait"].result())
            frames = [(e["src"], e["dst"]) for e in taken]
            if photo is not None:
                # into scratch frames: the buffer entries stay as rendered (resume re-renders them).  The scratch is allocated on this stream
                # and consumed on it by the augment launch below, so the allocator does not hand it out again before that launch has run.
                jit = ops.photometric_pairs([dict(src=s, dst=d, **p) for (s, d), p in zip(frames, photo)])
                frames = list(zip(jit["src"], jit["dst"]))
            samples = [dict(src=s, dst=d, flow=e["flow"], **p) for (s, d), e, p in zip(frames, taken, params)]
            if self.sparse is None:
                out = ops.augment_pairs(samples, size=self.crop)
            else:
                out = ops.augment_sparse_pairs([dict(s, quantize=self.sparse["quantize"]) for s in samples], size=self.crop)
            ready = torch.cuda.Event()
            ready.record(self.stream)
        self._batches += 1
        out["meta"] = [(e["job"]["name"], e["r"], e["job"]["obj_indices"][e["r"]], p["scale_x"], p["scale_y"], p["flip_h"], p.get("flip_v", 0), p["y0"], p["x0"])
                       for e, p in zip(taken, params)]
        if photo is not None:
            out["photo_meta"] = photo
        return out, ready

    # ---- teardown ------------------------------------------------------------------------------------------------------------------
    def _stop_producer(self):
        if self._producer is None:
            return
        self._stop.set()
        while self._producer.is_alive():
            try:
                self._q.get(timeout=0.05)
            except queue.Empty:
                pass
        self._producer.join()
        self._producer = None
        self._stop.clear()
        # the producer ran ahead of the consumer: rewind to what was delivered
        delivered = self._delivered
        self.stream.synchronize()
        self.load_state_dict(delivered)

    def close(self):
        if self._closed:
            return
        self._stop_producer()
        if self._pool is not None:
            self._pool.shutdown(wait=True)
            self._pool = None
        self.stream.synchronize()
        self.upload_stream.synchronize()
        self.tail.synchronize()
        self._buf, self._pending, self._resume_buf = [], [], []
        self._free_slots = self._busy_slots = collections.deque()
        self.lane = None
        self._closed = True

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:                                                  # noqa: BLE001
            pass
