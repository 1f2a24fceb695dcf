"""GPU: device-side image I/O against the NumPy restatement of Pillow's resampler (tests/resample_oracle.py, pinned to
PIL.Image.resize by test_resample_oracle_host.py) and the torch expressions of the three uint8 conversions.  Every
comparison is exact.  The kernels' outputs and workspace sit in guarded buffers (tests/guarded.py)."""
import functools

import numpy as np
import pytest
import torch
from PIL import Image

import image_compression_2_amd as ic2
from image_compression_2_amd import _native as nv
from image_compression_2_amd import image_io, ops

import resample_oracle as ro
from guarded import Guarded, _nan_bits

pytestmark = pytest.mark.gpu

FILL = 0x77


class GuardedU8:
    """`numel` uint8 elements prefilled with FILL between sentinel guards: a byte view of a Guarded int32 buffer (which
    has no one-byte sentinel).  The up to three bytes between the view's end and the guard must keep the prefill."""

    def __init__(self, numel, device):
        self.g = Guarded((numel + 3) // 4, torch.int32, device, fill=FILL * 0x01010101)
        raw = self.g.t.view(torch.uint8)
        self.t, self.tail = raw[:numel], raw[numel:]

    def intact(self):
        return self.g.intact() and bool((self.tail == FILL).all().item())


@functools.lru_cache(maxsize=None)
def _sources(h, w, c):
    """Three distinct uint8 [h][w][c] images: noise, 0 / 255 (both sides of the clip), noise."""
    return tuple(ro.make_image(h, w, c, kind, seed) for kind, seed in (("noise", 11), ("binary", 12), ("noise", 13)))


@functools.lru_cache(maxsize=None)
def _expected(h, w, c, oh, ow, f):
    """The oracle's [3][oh][ow][c] for _sources(h, w, c), computed once and shared."""
    out = np.stack([ro.resize(img, (oh, ow), f) for img in _sources(h, w, c)])
    out.setflags(write=False)
    return out


def _run_guarded(dev, images, sizes, c, oh, ow, name, lut):
    """ic2_resample_u8 through ops.py on the product's own records, with workspace and output in guarded buffers."""
    src = torch.cat([torch.from_numpy(i).reshape(-1) for i in images]).to(dev)
    arena, (recs, max_rows, total_rows) = image_io._plan(sizes, oh, ow, c, ro.FILTERS[name], dev)
    n = len(sizes)
    ws = GuardedU8(total_rows * ow * c, dev)
    if lut is None:
        out = GuardedU8(n * oh * ow * c, dev)
    else:
        out = Guarded(n * c * oh * ow, torch.float32, dev)
    ops.resample_u8(src, recs, arena.buf, ws.t, out.t, n, c, oh, ow, max_rows, total_rows, lut=lut)
    torch.cuda.synchronize()
    assert ws.intact() and out.intact(), "a guard element was overwritten"
    if lut is not None:
        assert not _nan_bits(out.t).any().item(), "an output element was not written"
    return out.t.view(n, oh, ow, c) if lut is None else out.t.view(n, c, oh, ow)


@pytest.mark.parametrize("c", [3, 1])
@pytest.mark.parametrize("name", sorted(ro.FILTERS))
@pytest.mark.parametrize("geom", ro.GEOMETRIES, ids=lambda g: "%dx%d-%dx%d" % g)
def test_uniform_batch_equals_the_oracle(cuda, geom, name, c):
    h, w, oh, ow = geom
    images = _sources(h, w, c)
    want = torch.from_numpy(_expected(h, w, c, oh, ow, ro.FILTERS[name]).copy())
    lut = ro.lut(c, 0.5, 0.5) if c == 1 else ro.lut(3, (0.5, 0.4, 0.6), (0.5, 0.25, 0.2))   # distinct per channel
    # uint8 HWC
    got = _run_guarded(cuda, images, [(h, w)] * 3, c, oh, ow, name, None)
    assert torch.equal(got.cpu(), want)
    # f32 NCHW through the table
    got = _run_guarded(cuda, images, [(h, w)] * 3, c, oh, ow, name, lut.to(cuda))
    want_f = torch.stack([lut[ch][want[..., ch].long()] for ch in range(c)], dim=1)
    assert got.shape == (3, c, oh, ow) and torch.equal(got.cpu().view(torch.int32), want_f.view(torch.int32))
    # the public calls give the same
    batch = torch.from_numpy(np.stack(images)).to(cuda)
    assert torch.equal(ic2.resize_u8(batch, (oh, ow), name).cpu(), want)
    mean, std = (0.5, 0.5) if c == 1 else ((0.5, 0.4, 0.6), (0.5, 0.25, 0.2))
    assert torch.equal(ic2.to_tensor(batch, (oh, ow), name, mean=mean, std=std).cpu().view(torch.int32),
                       want_f.view(torch.int32))


RAGGED = [(61, 47), (16, 16), (100, 75), (32, 40)]


def test_ragged_batch_equals_single_image_calls(cuda):
    images = [ro.make_image(h, w, 3, "noise" if i % 2 else "binary", 20 + i) for i, (h, w) in enumerate(RAGGED)]
    want = np.stack([ro.resize(img, (32, 32), ro.LANCZOS) for img in images])
    got = _run_guarded(cuda, images, RAGGED, 3, 32, 32, "lanczos", None).cpu()
    assert np.array_equal(got.numpy(), want)
    dev_imgs = [torch.from_numpy(i).to(cuda) for i in images]
    singles = torch.cat([ic2.resize_u8([t], 32) for t in dev_imgs])
    assert torch.equal(singles.cpu(), got)
    # one call on the list, from device tensors and from CPU tensors (one pinned upload)
    assert torch.equal(ic2.resize_u8(dev_imgs, (32, 32)).cpu(), got)
    assert torch.equal(ic2.resize_u8([torch.from_numpy(i) for i in images], 32, device=cuda).cpu(), got)
    lut = ro.lut(3)
    want_f = torch.stack([lut[ch][got[..., ch].long()] for ch in range(3)], dim=1)
    assert torch.equal(ic2.to_tensor(dev_imgs, 32).cpu().view(torch.int32), want_f.view(torch.int32))


# ------------------------------------------------------------------ f32 -> uint8
def _thresholds(mode):
    """The f32 nearest each x at which the conversion steps from code k - 1 to k, k = 0 .. 256."""
    k = np.arange(257, dtype=np.float64)
    x = {"eval": 2 * k / 255 - 1, "save_image": (k - 0.5) * 2 / 255 - 1, "reference": k / 127.5 - 1}[mode]
    return x.astype(np.float32)


@functools.lru_cache(maxsize=None)
def _probe_values():
    vals = [ro.lut(1)[0].numpy()]
    for mode in ("eval", "save_image", "reference"):
        t = _thresholds(mode)
        vals += [t, np.nextafter(t, np.float32(-np.inf)), np.nextafter(t, np.float32(np.inf))]
    vals.append(np.array([1.5, -1.5, np.inf, -np.inf, np.nan, 0.0, -0.0, 1.0, -1.0], dtype=np.float32))
    return torch.from_numpy(np.concatenate(vals).astype(np.float32))


def _expected_u8(x, mode):
    """The mode's torch expression on the CPU where it is defined, the stated saturation and NaN -> 0 elsewhere."""
    nan = torch.isnan(x)
    xs = torch.where(nan, torch.zeros_like(x), x)
    if mode == "eval":
        y = ((xs * 0.5 + 0.5).clamp(0, 1) * 255).to(torch.uint8)
    elif mode == "save_image":
        y = ((xs + 1) / 2).mul(255).add(0.5).clamp(0, 255).to(torch.uint8)
    else:
        u = (xs + 1.0) * 127.5
        inside = (u >= 0) & (u < 256)
        y = torch.where(inside, u, torch.zeros_like(u)).to(torch.uint8)   # trunc, as numpy astype(np.uint8)
        y = torch.where(u >= 256, torch.full_like(y, 255), y)
    return torch.where(nan, torch.zeros_like(y), y)


@pytest.mark.parametrize("mode", ["eval", "save_image", "reference"])
def test_to_uint8_equals_the_torch_expression(cuda, mode):
    """n = 2, c = 3, h = 5, w = 7 (35 pixels: no multiple of four, so byte and dword stores both run): all 256 table
    values, the f32 neighbours of every threshold of every mode, +-1.5, +-inf and NaN, 210 values per call."""
    vals = _probe_values()
    per = 2 * 3 * 5 * 7
    vals = torch.cat([vals, vals[:(-len(vals)) % per]])
    for chunk in vals.view(-1, 2, 3, 5, 7):
        y = GuardedU8(per, cuda)
        ops.image_to_u8(chunk.to(cuda), y.t, 2, 3, 5, 7, image_io._MODES[mode])
        torch.cuda.synchronize()
        assert y.intact()
        want = _expected_u8(chunk, mode).permute(0, 2, 3, 1).contiguous()
        assert torch.equal(y.t.cpu().view(2, 5, 7, 3), want)
        assert torch.equal(ic2.to_uint8(chunk.to(cuda), mode).cpu(), want)


@pytest.mark.parametrize("c", [1, 3])
def test_to_uint8_aligned_shape_and_round_trip(cuda, c):
    """16 x 16 (whole dwords): to_uint8(to_tensor(u8), "save_image") returns u8 for all 256 codes; "eval" and
    "reference" return the 63 codes the torch expressions return one lower."""
    u8 = torch.arange(256, dtype=torch.uint8).view(1, 16, 16, 1).repeat(2, 1, 1, c)
    u8[1] = u8[1].flip(0)
    x = ic2.to_tensor(u8.to(cuda))
    assert x.shape == (2, c, 16, 16)
    assert torch.equal(x.cpu(), ro.lut(c)[0][u8.long()].permute(0, 3, 1, 2))
    assert torch.equal(ic2.to_uint8(x, "save_image").cpu(), u8)
    lower = _expected_u8(ro.lut(1)[0], "eval").long() - torch.arange(256)
    assert int((lower != 0).sum()) == 63
    for mode in ("eval", "reference"):
        got = ic2.to_uint8(x, mode).cpu()
        assert torch.equal(got.long() - u8.long(), lower[u8.long()])


# ------------------------------------------------------------------ end to end
def test_image_batches_equal_pil_and_the_table(cuda, tmp_path):
    rng = np.random.default_rng(31)
    for i, (h, w) in enumerate([(40, 56), (64, 64), (33, 90), (120, 75), (64, 48)]):
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(tmp_path / f"img{i}.png")
    ds = ic2.ImageDataset(str(tmp_path), resolution=64)
    assert len(ds) == 5
    lut = ro.lut(3)
    want = []
    for path in ds.image_paths:
        r = np.asarray(Image.open(path).convert("RGB").resize((64, 64), Image.Resampling.LANCZOS))
        r = torch.from_numpy(r.copy()).long()
        want.append(torch.stack([lut[ch][r[..., ch]] for ch in range(3)]))
    batches = list(ic2.image_batches(ds, 2, cuda, workers=2))
    assert [tuple(b.shape) for b in batches] == [(2, 3, 64, 64), (2, 3, 64, 64), (1, 3, 64, 64)]
    assert all(b.is_cuda and b.dtype == torch.float32 for b in batches)
    got = torch.cat(batches).cpu()
    assert torch.equal(got.view(torch.int32), torch.stack(want).view(torch.int32))


def test_save_images_round_trip(cuda, tmp_path):
    u8 = torch.from_numpy(np.stack([ro.make_image(9, 11, 3, "noise", 40 + i) for i in range(2)]))
    paths = [str(tmp_path / f"o{i}.png") for i in range(2)]
    ic2.save_images(ic2.to_tensor(u8.to(cuda)), paths)
    for p, img in zip(paths, u8):
        assert np.array_equal(np.asarray(Image.open(p)), img.numpy())


# ------------------------------------------------------------------ graph capture
def test_resize_is_capturable(cuda):
    images = torch.from_numpy(np.stack(_sources(61, 47, 3))).to(cuda)
    eager = ic2.resize_u8(images, (16, 24))            # also caches the tables and records on the device
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = ic2.resize_u8(images, (16, 24))
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    assert torch.equal(out.cpu(), torch.from_numpy(_expected(61, 47, 3, 16, 24, ro.LANCZOS).copy()))
