"""Device-side image I/O: the uint8 ends of the reference's snippets, on the GPU.

Into the model, ``transforms.Compose([Resize(.., LANCZOS), ToTensor(), Normalize(.5, .5)])`` of ``ImageDataset``
(stylegan3_hvae_full.py:969-973) and of the README quick start: ``to_tensor`` / ``resize_u8`` run Pillow's 8-bit
resampler bit for bit (integer arithmetic on fixed-point coefficients, ic2_resample_u8) on a whole, possibly ragged,
batch of uint8 images and apply ToTensor + Normalize as a 256-entry table, so only uint8 bytes cross to the device.
Out of the model, ``to_uint8`` / ``save_images`` (ic2_image_to_u8) restate the three f32 -> uint8 conversions the
reference uses.  Only "save_image" inverts the table on all 256 codes; "eval" and "reference" return 63 codes one
lower.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes
import glob
import os
from collections import OrderedDict
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch
from torch.utils.data import Dataset

from . import _native as nv
from . import ops

__all__ = ["resample_tables", "normalize_table", "resize_u8", "to_tensor", "to_uint8", "save_images",
           "ImageDataset", "image_batches"]

_FILTERS = {"bilinear": nv.RESAMPLE_BILINEAR, "bicubic": nv.RESAMPLE_BICUBIC, "lanczos": nv.RESAMPLE_LANCZOS}
_MODES = {"eval": nv.U8_EVAL, "save_image": nv.U8_SAVE_IMAGE, "reference": nv.U8_REFERENCE}
_IDENTITY = -1          # filter code of an axis that keeps its size: Pillow skips the pass
_ONE = 1 << 22          # 1.0 in the tables' fixed point

_HOST_TABLES_MAX = 256  # host tables kept, least recently used dropped first
_ARENA_INTS = 1 << 20   # int32s of device table memory per device (a 1024 -> 256 Lanczos table is 6,912)
_RECORDS_MAX = 64       # device record sets kept per process


def _filter_code(resample):
    if isinstance(resample, str) and resample.lower() in _FILTERS:
        return _FILTERS[resample.lower()]
    if not isinstance(resample, str) and resample in _FILTERS.values():
        return int(resample)
    raise ValueError(f"resample must be one of {sorted(_FILTERS)} (or its IC2_RESAMPLE_* code), got {resample!r}")


_host_tables = OrderedDict()   # (in, out, code) -> (bounds, kk)


def _tables(in_size, out_size, code):
    key = (int(in_size), int(out_size), code)
    hit = _host_tables.get(key)
    if hit is not None:
        _host_tables.move_to_end(key)
        return hit
    if code == _IDENTITY:
        bounds = np.stack([np.arange(key[0]), np.ones(key[0])], axis=1).astype(np.int32)
        kk = np.full([key[0], 1], _ONE, dtype=np.int32)
    else:
        ks = nv.query("ic2_resample_ksize", *key)
        if ks <= 0:
            raise ValueError(f"resample_tables: sizes must be within [1, 16384], got {key[0]} -> {key[1]}")
        bounds = np.empty([key[1], 2], dtype=np.int32)
        kk = np.empty([key[1], ks], dtype=np.int32)
        nv.call("ic2_resample_coeffs", *key, bounds.ctypes.data_as(ctypes.c_void_p),
                kk.ctypes.data_as(ctypes.c_void_p))
    bounds.setflags(write=False)
    kk.setflags(write=False)
    _host_tables[key] = (bounds, kk)
    while len(_host_tables) > _HOST_TABLES_MAX:
        _host_tables.popitem(last=False)
    return bounds, kk


def resample_tables(in_size, out_size, resample="lanczos"):
    """One axis' table of Pillow's resampler for in_size -> out_size (ic2_resample_coeffs; host only): int32 arrays
    (bounds [out][2] = (first source index, taps), kk [out][ksize] = the taps' coefficients, 22 fraction bits).  The
    arrays are cached and read-only; their device copies live in a bounded per-device cache keyed by (in, out, filter,
    device), so a repeated size costs no upload."""
    return _tables(in_size, out_size, _filter_code(resample))


class _Arena:
    """The device copies of the tables one device uses: one int32 allocation filled front to back (the kernels address
    a table by its offset), dropped as a whole for a fresh one when full.  Memory is only ever appended to."""

    count = 0

    def __init__(self, device, ints):
        _Arena.count += 1
        self.gen = _Arena.count   # names the arena in the record cache (an id() could come back)
        self.buf = torch.empty([ints], dtype=torch.int32, device=device)
        self.used = 0
        self.offsets = {}   # (in, out, code) -> offset in int32s


_arenas = {}                # device -> _Arena
_records = OrderedDict()    # (arena generation, sizes, oh, ow, c, code) -> (recs, max_rows, total_rows)
_luts = OrderedDict()       # (c, mean, std, device) -> [c][256] f32


def _refuse_capture(what):
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError(f"image_io: {what} would be uploaded during a graph capture (a replay would re-read host "
                           "memory that is gone by then); run the same call once before capturing")


def _upload(host, dst):
    """dst (device) <- host (a CPU tensor) through pinned memory, not blocking the host."""
    dst.copy_(host.pin_memory(), non_blocking=True)


def _device_tables(keys, device):
    """(arena, {key: offset}) with every key's table resident in the arena."""
    need = {k: 2 * k[1] + k[1] * _tables(*k)[1].shape[1] for k in keys}
    arena = _arenas.get(device)
    missing = [k for k in need if arena is None or k not in arena.offsets]
    if missing and (arena is None or arena.used + sum(need[k] for k in missing) > arena.buf.numel()):
        _refuse_capture("resample tables")
        arena = _arenas[device] = _Arena(device, max(_ARENA_INTS, sum(need.values())))
        missing = list(need)
    if missing:
        _refuse_capture("resample tables")
        host = np.concatenate([a.reshape(-1) for k in missing for a in _tables(*k)])
        _upload(torch.from_numpy(host), arena.buf[arena.used:arena.used + host.size])
        for k in missing:
            arena.offsets[k] = arena.used
            arena.used += need[k]
    return arena, {k: arena.offsets[k] for k in need}


def _plan(sizes, oh, ow, c, code, device):
    """Device records and row counts of a batch whose sources are packed back to back in `sizes` order."""
    def axis_key(n_in, n_out):
        return (n_in, n_out, _IDENTITY if n_in == n_out else code)

    keys = {axis_key(w, ow) for _, w in sizes} | {axis_key(h, oh) for h, _ in sizes}
    arena, offs = _device_tables(keys, device)
    rkey = (arena.gen, tuple(sizes), oh, ow, c, code)
    hit = _records.get(rkey)
    if hit is not None:
        _records.move_to_end(rkey)
        return arena, hit
    _refuse_capture("image records")
    rec = np.zeros([len(sizes), 9], dtype=np.int64)
    src_off = ws_off = max_rows = 0
    for i, (h, w) in enumerate(sizes):
        kx, ky = axis_key(w, ow), axis_key(h, oh)
        yb = _tables(*ky)[0]
        y0 = int(yb[0, 0])
        rows = int(yb[-1, 0]) + int(yb[-1, 1]) - y0
        rec[i] = (src_off, h, w, offs[kx], offs[ky], _tables(*kx)[1].shape[1], _tables(*ky)[1].shape[1], ws_off, y0)
        src_off += h * w * c
        ws_off += rows * ow * c
        max_rows = max(max_rows, rows)
    recs = torch.empty([len(sizes), 9], dtype=torch.int64, device=device)
    _upload(torch.from_numpy(rec), recs)
    hit = _records[rkey] = (recs, max_rows, ws_off // (ow * c))
    while len(_records) > _RECORDS_MAX:
        _records.popitem(last=False)
    return arena, hit


def _device_of(device):
    if not torch.cuda.is_available():
        nv.require_gpu(torch.empty(0))   # raises: ROCm devices only
    device = torch.device("cuda" if device is None else device)
    return torch.device("cuda", torch.cuda.current_device()) if device.index is None else device


def _pack(images, device):
    """(src blob on the device, [(h, w)], c) of a uint8 [N,H,W,C] device tensor or a list of [H,W,C] uint8 tensors."""
    if isinstance(images, torch.Tensor):
        nv.require_gpu(images)
        if images.dtype is not torch.uint8 or images.dim() != 4 or images.shape[0] == 0:
            raise ValueError(f"expected a uint8 [N,H,W,C] tensor, got {images.dtype} {tuple(images.shape)}")
        n, h, w, c = images.shape
        return images, [(h, w)] * n, c
    images = list(images)
    if not images:
        raise ValueError("expected at least one image")
    for t in images:
        if not isinstance(t, torch.Tensor) or t.dtype is not torch.uint8 or t.dim() != 3 or \
                t.shape[2] != images[0].shape[2] or t.device != images[0].device:
            raise ValueError("expected a list of uint8 [H,W,C] tensors with one channel count, on one device")
    sizes = [(int(t.shape[0]), int(t.shape[1])) for t in images]
    c = int(images[0].shape[2])
    if images[0].is_cuda:
        return torch.cat([t.reshape(-1) for t in images]), sizes, c
    device = _device_of(device)
    _refuse_capture("the source images")
    blob = torch.empty([sum(h * w * c for h, w in sizes)], dtype=torch.uint8).pin_memory()
    off = 0
    for t in images:
        blob[off:off + t.numel()] = t.reshape(-1)
        off += t.numel()
    return blob.to(device, non_blocking=True), sizes, c


def _resample(images, size, resample, lut, device):
    src, sizes, c = _pack(images, device)
    if c not in (1, 3):
        raise ValueError(f"images must have 1 or 3 channels, got {c}")
    if size is None:
        if len(set(sizes)) != 1:
            raise ValueError("size=None needs images of one size")
        size = sizes[0]
    oh, ow = (int(size), int(size)) if isinstance(size, int) else (int(size[0]), int(size[1]))
    dev, n = src.device, len(sizes)
    arena, (recs, max_rows, total_rows) = _plan(sizes, oh, ow, c, _filter_code(resample), dev)
    ws = torch.empty([total_rows * ow * c], dtype=torch.uint8, device=dev)
    if lut is None:
        out = torch.empty([n, oh, ow, c], dtype=torch.uint8, device=dev)
    else:
        out = torch.empty([n, c, oh, ow], dtype=torch.float32, device=dev)
    return ops.resample_u8(src, recs, arena.buf, ws, out, n, c, oh, ow, max_rows, total_rows, lut=lut)


def resize_u8(images, size, resample="lanczos", device=None):
    """PIL.Image.resize((ow, oh), resample) of every image, bit for bit: `images` a uint8 [N,H,W,C] device tensor, or
    a list of [H,W,C] uint8 tensors of any sizes (CPU tensors are packed into one pinned blob and uploaded to `device`
    with one non-blocking copy) -> uint8 [N,oh,ow,C] on the device.  size: (oh, ow) or one int for both; C is 1 or 3.
    Capturable once the same call has run before (its tables and records are then cached on the device)."""
    return _resample(images, size, resample, None, device)


def normalize_table(c, mean=0.5, std=0.5):
    """ToTensor then Normalize(mean, std) of every uint8 code, [c][256] f32 on the CPU, in torch's own ops (the
    reference's arithmetic by construction).  mean / std: a scalar or one entry per channel."""
    mean = tuple(float(m) for m in (mean if isinstance(mean, (tuple, list)) else [mean] * c))
    std = tuple(float(s) for s in (std if isinstance(std, (tuple, list)) else [std] * c))
    if len(mean) != c or len(std) != c:
        raise ValueError(f"mean and std must be scalars or have one entry per channel ({c})")
    base = torch.arange(256).float().div(255)
    return torch.stack([base.sub(m).div(s) for m, s in zip(mean, std)]).contiguous()


def _lut(c, mean, std, device):
    key = (c, str(mean), str(std), device)
    hit = _luts.get(key)
    if hit is None:
        _refuse_capture("the normalisation table")
        hit = _luts[key] = normalize_table(c, mean, std).to(device)
        while len(_luts) > 16:
            _luts.popitem(last=False)
    return hit


def to_tensor(images, size=None, resample="lanczos", mean=0.5, std=0.5, device=None):
    """Resize((oh, ow), resample) -> ToTensor -> Normalize(mean, std) of a batch (inputs as resize_u8 takes them) ->
    f32 [N,C,oh,ow].  size None: no resize (images of one size).  The normalisation is a [C][256] table built with
    torch's own ops, arange(256).float().div(255).sub(mean).div(std)."""
    if isinstance(images, torch.Tensor):
        dev, c = images.device, images.shape[-1]
    else:
        images = list(images)
        first = images[0] if images else None
        if not isinstance(first, torch.Tensor) or first.dim() != 3:
            raise ValueError("expected a uint8 [N,H,W,C] tensor or a non-empty list of [H,W,C] uint8 tensors")
        dev, c = (first.device if first.is_cuda else _device_of(device)), first.shape[2]
    if dev.type != "cuda":
        nv.require_gpu(images)
    return _resample(images, size, resample, _lut(int(c), mean, std, dev), dev)


def to_uint8(x, mode="save_image"):
    """The model's f32 [N,C,H,W] output as uint8 [N,H,W,C] (ic2_image_to_u8).  mode "eval": the metrics' conversion,
    trunc(clamp(x*0.5+0.5, 0, 1)*255) (hvae_training.py:368-388); "save_image": torchvision.utils.save_image((x+1)/2),
    rounding, the one that returns to_tensor's input for all 256 codes; "reference": save_tensor_as_image's
    trunc((x+1)*127.5), saturated outside [0, 256).  NaN gives 0."""
    if mode not in _MODES:
        raise ValueError(f"mode must be one of {sorted(_MODES)}, got {mode!r}")
    nv.require_gpu(x)
    if x.dtype is not torch.float32 or x.dim() != 4 or x.numel() == 0:
        raise ValueError(f"expected a non-empty f32 [N,C,H,W] tensor, got {x.dtype} {tuple(x.shape)}")
    n, c, h, w = x.shape
    y = torch.empty([n, h, w, c], dtype=torch.uint8, device=x.device)
    return ops.image_to_u8(x, y, n, c, h, w, _MODES[mode])


def save_images(x, paths, mode="save_image"):
    """Write the batch x (f32 [N,C,H,W], C 1 or 3) to `paths` (one per image): one conversion launch, one
    device -> host copy of the uint8 batch, then PIL's encoder per file."""
    from PIL import Image
    paths = list(paths)
    if len(paths) != x.shape[0]:
        raise ValueError(f"{x.shape[0]} images, {len(paths)} paths")
    if x.shape[1] not in (1, 3):
        raise ValueError(f"images must have 1 or 3 channels, got {x.shape[1]}")
    u8 = to_uint8(x, mode).cpu().numpy()
    for img, path in zip(u8, paths):
        Image.fromarray(img[..., 0] if img.shape[2] == 1 else img).save(path)


class ImageDataset(Dataset):
    """The reference's ImageDataset (stylegan3_hvae_full.py:936-998: constructor, file discovery, decode-error
    fallback) with the transform moved to the device: __getitem__ returns the decoded RGB image as a uint8 [H,W,3] CPU
    tensor at its own size, and `image_batches` resizes and normalises whole batches on the GPU.  On a decode error
    the next image is returned; after the last one, zeros (uint8 [resolution, resolution, 3]; the reference's f32
    zeros have no uint8 code)."""

    def __init__(self, image_folder, resolution=256, is_imagenet=False, recursive=True,
                 file_extensions=(".png", ".jpg", ".jpeg")):
        self.image_folder = image_folder
        self.resolution = resolution
        self.is_imagenet = is_imagenet
        self.file_extensions = tuple(file_extensions)
        self.image_paths = []
        if is_imagenet or recursive:
            for root, _, files in os.walk(image_folder):
                for file in files:
                    if file.lower().endswith(self.file_extensions):
                        self.image_paths.append(os.path.join(root, file))
        else:
            for ext in self.file_extensions:
                self.image_paths.extend(glob.glob(os.path.join(image_folder, f"*{ext}")))
                self.image_paths.extend(glob.glob(os.path.join(image_folder, f"*{ext.upper()}")))
        print(f"Found {len(self.image_paths)} images in {image_folder}")

    def __len__(self):
        return len(self.image_paths)

    def __getitem__(self, idx):
        from PIL import Image
        while idx < len(self.image_paths):
            try:
                with Image.open(self.image_paths[idx]) as img:
                    return torch.from_numpy(np.array(img.convert("RGB"), dtype=np.uint8))
            except Exception as e:
                print(f"Error loading image {self.image_paths[idx]}: {e}")
                idx += 1
        return torch.zeros(self.resolution, self.resolution, 3, dtype=torch.uint8)


def image_batches(dataset, batch_size, device=None, resample="lanczos", mean=0.5, std=0.5, shuffle=False,
                  drop_last=False, generator=None, workers=0):
    """Iterate `dataset` (an ImageDataset, or anything with `resolution` whose items are uint8 [H,W,C] CPU tensors) as
    f32 [B,C,resolution,resolution] device batches: the reference's DataLoader over Resize(LANCZOS) + ToTensor +
    Normalize, with the transform as one `to_tensor` call per batch.  workers > 0 decodes the batch's files on that
    many threads.  There is no CPU fallback."""
    device = _device_of(device)
    order = torch.randperm(len(dataset), generator=generator).tolist() if shuffle else list(range(len(dataset)))
    res = (dataset.resolution, dataset.resolution)
    pool = ThreadPoolExecutor(workers) if workers > 0 else None
    try:
        for i in range(0, len(order), batch_size):
            idx = order[i:i + batch_size]
            if drop_last and len(idx) < batch_size:
                break
            batch = list(pool.map(dataset.__getitem__, idx)) if pool else [dataset[j] for j in idx]
            yield to_tensor(batch, size=res, resample=resample, mean=mean, std=std, device=device)
    finally:
        if pool:
            pool.shutdown()
