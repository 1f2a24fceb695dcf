"""ic2_conv_wino on flat tiles (csrc/wino.hip wx_slot: the tile's th x twp <= 128 pair slots numbered row-major and
cut into 16-lane blocks that wrap across tile rows).  A tile only moves which lane computes which output pair: the K
order and the output transform of every output stay, so each forced flat tile is compared bit for bit with the same
conv under IC2_WINO_FLAT=0 (row-blocked tiles only), and with an fp64 conv within test_gpu_wino.py's bound.  The knobs
are read once per process, so every knob setting runs in a child process (all of them side by side, once per module)."""
import json
import os
import subprocess
import sys
import tempfile

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

GUARD = 8192
SENTINEL = -1234.5

# name: n, output width, output height, forced twp, forced th, cin, cin_p, cout, cout_p   (pad 2: input = output - 2)
CASES = {
    # 35 slots in 3 blocks, every block spans 3-4 rows; odd width, ragged last tile in x and y; two K blocks (the halo
    # buffers swap); two o-tiles, the second partial
    "c1": (2, 15, 15, 5, 7, 60, 64, 130, 160),
    "c2": (1, 42, 12, 21, 6, 32, 32, 32, 32),    # 126 of 128 slots, all 8 blocks used
    "c3": (1, 50, 10, 25, 5, 90, 96, 32, 32),    # the halo at 364 of 384 rows
    "c4": (1, 6, 40, 3, 38, 32, 32, 32, 32),     # a tall tile wrapping every 3 lanes
}
# output layout, output dtype, blocked input, activation
VARIANTS = {"nhwc": ("NHWC", "float16", False, True), "nhwc16": ("NHWC16", "float16", False, True),
            "nchw_f32": ("NCHW", "float32", False, True), "nhwc_bin": ("NHWC", "float16", True, True),
            "nhwc16_bin": ("NHWC16", "float16", True, True), "nchw_f32_bin": ("NCHW", "float32", True, True),
            "nhwc_noact": ("NHWC", "float16", False, False), "nhwc16_noact": ("NHWC16", "float16", False, False)}
CASE_VARIANTS = {"c1": list(VARIANTS), "c2": ["nhwc16"], "c3": ["nhwc16_bin"], "c4": ["nhwc"]}


def _child(case_names, reference, out_path):
    """Runs in the child: every variant of the named cases; outputs (with their guard bands), the plan name and, with
    `reference`, the errors of the Winograd and the direct conv against fp64."""
    from image_compression_2_amd import _native as nv
    dev = torch.device("cuda", 0)
    res = {}
    for name in case_names:
        n, wo, ho, _, _, ci, cip, co, cop = CASES[name]
        h, w_, pad = ho - 2, wo - 2, 2
        g = torch.Generator().manual_seed(17)
        x = torch.zeros(n, h, w_, cip)
        x[..., :ci] = torch.randn(n, h, w_, ci, generator=g)
        x = x.to(dev, torch.float16)
        w = torch.randn(co, ci, 3, 3, generator=g).to(dev)
        osc = ((torch.rand(n, cop, generator=g) + 0.5) / (9 * ci) ** 0.5).to(dev)
        bias = (torch.randn(cop, generator=g) * 0.1).to(dev)
        xb = x.reshape(n, h, w_, cip // 16, 16).permute(0, 3, 1, 2, 4).contiguous()
        st = nv.stream_of(x)
        u = torch.empty(cop, 3, 4, cip, device=dev, dtype=torch.float16)
        wp = torch.empty(cop, 3, 3, cip, device=dev, dtype=torch.float16)
        nv.call("ic2_pack_weight_wino", nv.ptr(w), co, ci, cop, cip, 1, 1.0, nv.ptr(u), nv.F16, st)
        nv.call("ic2_pack_weight", nv.ptr(w), co, ci, 3, 3, cop, cip, 1, 1.0, nv.ptr(wp), nv.F16, None, st)
        plan = nv.wino_plan(n, h, w_, cip, cop, pad)
        for vname in CASE_VARIANTS[name]:
            lay, dt, blocked, act_on = VARIANTS[vname]
            slope, gain, clamp, mul = (0.2, 1.4142135, 2.5, 0.75) if act_on else (0.0, 1.0, -1.0, 1.0)
            layout, out_dt = getattr(nv, lay), getattr(torch, dt)
            shape = {"NCHW": [n, co, ho, wo], "NHWC16": [n, cop // 16, ho, wo, 16], "NHWC": [n, ho, wo, cop]}[lay]
            numel = 1
            for d in shape:
                numel *= d

            def buf():
                base = torch.full([GUARD + numel + GUARD], SENTINEL, device=dev, dtype=out_dt)
                base[GUARD:GUARD + numel] = 7.0
                return base, base[GUARD:GUARD + numel].view(shape)
            base, y = buf()
            act = int(act_on) | (nv.act_in_layout(nv.NHWC16) if blocked else 0)
            with torch.no_grad():
                nv.conv_wino(nv.ptr(xb if blocked else x), nv.ptr(u), nv.ptr(y), nv.F16, nv.dtype_code(out_dt), n, h, w_,
                             cip, cop, co, pad, ho, wo, nv.ptr(osc), nv.ptr(bias), act, slope, gain, clamp, mul, layout,
                             st)
            torch.cuda.synchronize()
            row = {"plan": plan, "base": base.cpu(), "bias": bias.cpu()}
            if reference:
                _, yd = buf()
                with torch.no_grad():
                    nv.conv_igemm(nv.ptr(x), nv.ptr(wp), nv.ptr(yd), nv.F16, nv.dtype_code(out_dt), n, h, w_, cip, cop,
                                  co, 3, 3, pad, ho, wo, nv.ptr(osc), nv.ptr(bias), int(act_on), slope, gain, clamp, mul,
                                  layout, st, dev)
                torch.cuda.synchronize()
                wn = (w * w.square().mean([1, 2, 3], keepdim=True).rsqrt()).double()
                ref = F.conv2d(x[..., :ci].double().permute(0, 3, 1, 2), wn, padding=pad)
                ref = ref * osc[:, :co, None, None].double() + bias[None, :co, None, None].double()
                if act_on:
                    ref = (torch.where(ref < 0, ref * slope, ref) * gain).clamp(-clamp, clamp) * mul
                scale = ref.abs().max().item()
                row["e_w"] = (_as_nchw(y, lay, n, cop, ho, wo)[:, :co].double() - ref).abs().max().item() / scale
                row["e_d"] = (_as_nchw(yd, lay, n, cop, ho, wo)[:, :co].double() - ref).abs().max().item() / scale
            res[f"{name}/{vname}"] = row
    torch.save(res, out_path)


def _as_nchw(y, lay, n, cop, ho, wo):
    if lay == "NCHW":
        return y
    if lay == "NHWC16":
        return y.permute(0, 1, 4, 2, 3).reshape(n, cop, ho, wo)
    return y.permute(0, 3, 1, 2)


@pytest.fixture(scope="module")
def runs(cuda):
    """{"base": the IC2_WINO_FLAT=0 outputs of every case, case name: its forced flat tile's} from five children."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with tempfile.TemporaryDirectory() as tmp:
        procs = {}
        jobs = {"base": (list(CASES), False, {"IC2_WINO_FLAT": "0"})}
        for name, c in CASES.items():
            jobs[name] = ([name], True, {"IC2_WINO_FLAT": "2", "IC2_WINO_TWP": str(c[3]), "IC2_WINO_TH": str(c[4])})
        for tag, (names, reference, env) in jobs.items():
            out = os.path.join(tmp, tag + ".pt")
            code = (f"import sys; sys.path.insert(0, {root!r}); from tests.test_gpu_wino_flat import _child; "
                    f"_child({json.dumps(names)}, {reference!r}, {out!r})")
            procs[tag] = (out, subprocess.Popen([sys.executable, "-c", code], env=dict(os.environ, IC2_DEV="1", **env),
                                                stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
        res = {}
        for tag, (out, p) in procs.items():
            log, _ = p.communicate(timeout=600)
            assert p.returncode == 0, f"child {tag}: {log[-4000:]}"
            res[tag] = torch.load(out)
    return res


@pytest.mark.parametrize("key", [f"{c}/{v}" for c in CASES for v in CASE_VARIANTS[c]])
def test_flat_tile_is_bit_identical_and_matches_fp64(runs, key):
    name = key.split("/")[0]
    _, _, _, twp, th = CASES[name][:5]
    flat, base = runs[name][key], runs["base"][key]
    assert flat["plan"] == f"wino_fx_o128_p{twp}x{th}w_f16", flat["plan"]
    assert not base["plan"].endswith("w_f16"), base["plan"]
    print(f"[wino flat] {key}: rel err wino {flat['e_w']:.2e}, direct {flat['e_d']:.2e}")
    # every stored element and both guard bands, bit for bit
    assert torch.equal(flat["base"].view(torch.uint8), base["base"].view(torch.uint8))
    # test_gpu_wino.py's bound
    assert flat["e_w"] < 4e-3 and flat["e_w"] <= 4 * flat["e_d"] + 1e-4, (flat["e_w"], flat["e_d"])


@pytest.mark.parametrize("vname", ["nhwc_noact", "nhwc16_noact"])
def test_flat_tile_leaves_padding_channels_and_bounds(runs, vname):
    """Case 1 stored into a view inside a sentinel-filled buffer: both guards bit-unchanged, every valid output
    written, and the padded output channels 130..159 (zero U rows) hold 0 * acc * oscale + bias = the f16 bias."""
    n, wo, ho, _, _, _, _, co, cop = CASES["c1"]
    row = runs["c1"][f"c1/{vname}"]
    b = row["base"]
    numel = n * ho * wo * cop
    assert (b[:GUARD] == SENTINEL).all() and (b[GUARD + numel:] == SENTINEL).all(), "store outside the output tensor"
    shape = [n, cop // 16, ho, wo, 16] if vname == "nhwc16_noact" else [n, ho, wo, cop]
    y = _as_nchw(b[GUARD:GUARD + numel].view(shape), VARIANTS[vname][0], n, cop, ho, wo).float()
    assert not (y[:, :co] == 7.0).any(), "a valid output was not written"
    pad_ref = row["bias"][co:].to(torch.float16).float()[None, :, None, None].expand(n, cop - co, ho, wo)
    assert torch.equal(y[:, co:], pad_ref)
