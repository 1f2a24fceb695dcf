"""Every conv launch-plan instance against the fp64 convolution of a small-integer lattice, bit for bit.

tests/conv_lattice.py holds the operands, the reference, the three epilogues and the case table, and derives why a
correct instance must reproduce the reference exactly (integers below 2^24 in any summation order; dyadic epilogue
constants).  Here each (knob environment, operand dtype) runs in one child process (the knobs are read once per
process): the child asserts that the row still runs the instance it declares, launches through the C ABI into a
NaN-prefilled view between sentinel guard bands and requires, per launch: guards intact, no NaN left,
torch.equal(got, expected) over the whole tensor (padded channels hold epilogue(bias)).  Split forms also run without
their workspace (unsplit: the same bits); hg4, ToRGB and Winograd rows also run on channel-blocked input (the same
bits).  The child reports every failing row and ends at the first HIP error.

Rounding tier.  The lattice cannot see a loss of precision that keeps integers intact (f16 intermediates in Winograd),
so one small row per kernel family also runs Gaussian operands (rounded to the storage type) with a Gaussian `linear`
epilogue, f32 and 16-bit output, against the fp64 reference per element:
    |got - ref| <= K eps B + eps_out |ref|,   B = |oscale| conv(|x|, |w|) + |bias|
(Winograd: B through |B^T|, |G|, |A^T|), eps = 2^-24 for the direct kernels (exact products, f32 sums), 2^-11 for
Winograd (U and V rounded to f16), eps_out = 2^-8 / 2^-11 / 2^-24 for bf16 / f16 / f32 output.
K per family: derived count of roundings / measured max (|got - ref| - eps_out |ref|) / (eps B) on the MI355X / bar,
the bar at most min(derived, 2 x measured); the figures are recorded in profiles/r18_conv_lattice.txt.
  derived, direct kernels: a sum of kh kw cin_p products in any order rounds at most once per addition, plus the
    oscale product and the bias sum: K_len + 2 (s3a: 290, s3b: 578, h81_51 and hc32_32: 866 / 290).
  derived, Winograd: one f16 rounding of U = G w and one of V = B^T d per product (2), plus the f32 sums in units of
    2^-11: (3 cin_p + 5) 2^-13 (w64_96: 2.03).
  measured / bar:
    igemm         (igemm_128x128, s3a, bf16)              measured 0.776, bar 1.55
    igemm_splitk  (igemm_128x128_splitk_f16, s3b, f16)    measured 0.825, bar 1.65
    igemm8        (igemm8_og2 forced, s3b, bf16)          measured 1.205, bar 2.41
    hg4           (hg4_o64_w16_s4_f16, h81_51, f16)       measured 1.624, bar 3.25
    hconv         (hconv_32_32, hc32_32, bf16)            measured 1.713, bar 3.43
    f32           (igemm_f32_128x128, s3a, f32)           measured 3.163, bar 6.33
    wino          (wino_fx_o128_p16x7_f16, w64_96, f16)   measured 0.094, bar 0.188
  (Winograd's B bounds every product through the absolute transforms, so its measured ratio is far below the count.)
"""
import os
import subprocess
import sys
import tempfile

import pytest
import torch

import conv_lattice as cl

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _k_derived(family):
    _, rid, _ = cl.ROUNDING[family]
    r = cl.ROWS[rid]
    return 2 + (3 * r.cin_p + 5) * 2.0 ** -13 if family == "wino" else r.k * r.k * r.cin_p + 2.0


K_DERIVED = {f: _k_derived(f) for f in cl.ROUNDING}
# measured on the MI355X (profiles/r18_conv_lattice.txt)
K_MEASURED = {"igemm": 0.7755, "igemm_splitk": 0.8248, "igemm8": 1.2053, "hg4": 1.6237, "hconv": 1.7126, "f32": 3.1633,
              "wino": 0.0942}
K_BAR = {f: min(K_DERIVED[f], 2 * K_MEASURED[f]) for f in cl.ROUNDING}


def _launcher(nv, dev, rid, dtype, xd, wd):
    r = cl.ROWS[rid]
    ho, wo = r.h + 2 * r.pad - r.k + 1, r.w + 2 * r.pad - r.k + 1
    st = nv.stream_of(xd)
    dt = cl.DTYPE_CODE[dtype]

    def launch(x, y, epi, odt, lay, osc, bias, in_blocked=False, no_ws=False):
        p = cl.EPILOGUES[epi]
        act = p["act"] | (nv.act_in_layout(nv.NHWC16) if in_blocked else 0)
        tail = (nv.ptr(osc), nv.ptr(bias), act, p["slope"], p["gain"], p["clamp"], p["out_mul"], lay)
        if rid in cl.WINO:
            nv.conv_wino(nv.ptr(x), nv.ptr(wd), nv.ptr(y), nv.F16, odt, r.n, r.h, r.w, r.cin_p, r.cout_p, r.cout_valid,
                         r.pad, ho, wo, *tail, st)
            return
        head = (nv.ptr(x), nv.ptr(wd), nv.ptr(y), dt, odt, r.n, r.h, r.w, r.cin_p, r.cout_p, r.cout_valid, r.k, r.k,
                r.pad, ho, wo)
        if no_ws:   # a split form without its workspace runs unsplit (ic2ops.h)
            nv.call("ic2_conv_igemm_ws", *head, *tail, None, 0, st)
        else:
            nv.conv_igemm(*head, *tail, st, dev)
    return launch


def _device_operands(nv, dev, rid, dtype, x, w):
    """(x NHWC on the device in the operand dtype, the kernel's weight operand)."""
    r = cl.ROWS[rid]
    td = cl.TORCH_DTYPE[dtype]
    xd = x.to(td).to(dev)
    if rid not in cl.WINO:
        return xd, w.to(td).to(dev)
    w4 = cl.wino_weight_oihw(w, r).to(dev)
    u = torch.empty(r.cout_p, 3, 4, r.cin_p, device=dev, dtype=torch.float16)
    nv.call("ic2_pack_weight_wino", nv.ptr(w4), r.cout_valid, r.cin, r.cout_p, r.cin_p, 0, 1.0, nv.ptr(u), nv.F16,
            nv.stream_of(xd))
    torch.cuda.synchronize()
    return xd, u


def _plan_of(nv, rid, dtype):
    r = cl.ROWS[rid]
    if rid in cl.WINO:
        return nv.wino_plan(r.n, r.h, r.w, r.cin_p, r.cout_p, r.pad)
    return nv.conv_plan(*cl.plan_query(rid, dtype))


def _child(env, dtype, cache_dir):
    """Runs in the child: every row of PLAN[env] with operand dtype `dtype`.  Mismatches are collected and reported
    together; a HIP error (a RuntimeError from the call or the synchronize) ends the child at once."""
    from image_compression_2_amd import _native as nv
    from test_gpu_act_blocked import guarded, guards_intact, to_blocked
    dev = torch.device("cuda", 0)
    bad = []
    for rid in cl.PLAN[env]:
        r = cl.ROWS[rid]
        declared, name = cl.plan_name(env, rid, dtype), _plan_of(nv, rid, dtype)
        if name != declared:
            bad.append(f"{rid}: the plan is {name}, the row declares {declared}")
            continue
        x, w = cl.operands(rid)
        xd, wd = _device_operands(nv, dev, rid, dtype, x, w)
        launch = _launcher(nv, dev, rid, dtype, xd, wd)
        acc = cl.conv_acc(rid, cache_dir)
        for vi, (epi, odt, lay) in enumerate(cl.variants(rid, dtype)):
            osc, bias = cl.epilogue_params(rid, epi, acc)
            exp = cl.expected(cl.apply_epilogue(acc, epi, osc, bias), odt, lay, r.cout_valid)
            oscd, biasd = (None, None) if osc is None else (osc.to(dev), bias.to(dev))
            runs = [("", dict())]
            if vi == 0 and (declared.endswith(("_splitk", "_splitk_f16")) or "_tail" in declared):
                runs.append((" without workspace", dict(no_ws=True)))
            if vi == 0 and declared.startswith(("hg4_", "torgb", "wino_")):
                runs.append((" blocked input", dict(in_blocked=True)))
            for tag, kw in runs:
                base, y = guarded(list(exp.shape), cl.OUT_TORCH[odt], dev)
                xin = to_blocked(xd) if kw.get("in_blocked") else xd
                launch(xin, y, epi, odt, lay, oscd, biasd, **kw)
                torch.cuda.synchronize()
                where = f"{rid} [{declared}] {epi} out dtype {odt} layout {lay}{tag}"
                if not guards_intact(base, y.numel()):
                    bad.append(f"{where}: store outside the output tensor")
                got = y.cpu()
                if torch.isnan(got).any():
                    bad.append(f"{where}: {int(torch.isnan(got).sum())} elements were not written")
                diff = cl.first_difference(got, exp, lay)
                if diff:
                    bad.append(f"{where}: {diff}")
    assert not bad, "%d failures:\n%s" % (len(bad), "\n".join(bad[:40]))
    print(f"[conv-lattice] {env} {dtype}: {len(cl.PLAN[env])} rows bit-exact")


def _child_rounding(family):
    """Runs in the child: the rounding tier of one family (module docstring)."""
    from image_compression_2_amd import _native as nv
    env, rid, dtype = cl.ROUNDING[family]
    r = cl.ROWS[rid]
    dev = torch.device("cuda", 0)
    assert _plan_of(nv, rid, dtype) == cl.plan_name(env, rid, dtype)
    c = cl.gaussian_case(rid, dtype)
    xd, wd = _device_operands(nv, dev, rid, dtype, c["x"], c["w"])
    launch = _launcher(nv, dev, rid, dtype, xd, wd)
    oscd, biasd = c["oscale"].to(dev), c["bias"].to(dev)
    eps = cl.EPS.get(family, 2.0 ** -24)
    worst, bad = 0.0, []
    for odt in (cl.F32, cl.BF16 if dtype != "f16" else cl.F16):
        y = torch.full(list(c["ref"].shape), float("nan"), dtype=cl.OUT_TORCH[odt], device=dev)
        launch(xd, y, "linear", odt, cl.NHWC, oscd, biasd)
        torch.cuda.synchronize()
        ref, B = c["ref"][..., :r.cout_valid], c["B"][..., :r.cout_valid]
        err = (y.cpu().double()[..., :r.cout_valid] - ref).abs()
        ratio = ((err - cl.EPS_OUT[odt] * ref.abs()).clamp_min(0) / (eps * B)).max().item()
        worst = max(worst, ratio)
        print(f"[conv-lattice rounding] {family} out dtype {odt}: max (err - eps_out |ref|) / (eps B) = {ratio:.4f}")
        over = err > K_BAR[family] * eps * B + cl.EPS_OUT[odt] * ref.abs()
        if not torch.isfinite(err).all() or over.any():
            bad.append(f"out dtype {odt}: {int(over.sum())} elements over the bound, ratio {ratio:.4f}")
    print(f"[conv-lattice rounding] {family}: measured {worst:.4f}, bar {K_BAR[family]:.4g}, "
          f"derived {K_DERIVED[family]:.4g}")
    assert not bad, bad


def _run_child(call, env):
    code = (f"import sys; sys.path.insert(0, {ROOT!r}); sys.path.insert(0, {os.path.join(ROOT, 'tests')!r}); "
            f"import test_gpu_conv_lattice as t; t.{call}")
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, IC2_DEV="1", **cl.ENVS[env]),
                       capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-6000:] + r.stderr[-6000:]


@pytest.fixture(scope="module")
def cache_dir():
    """The fp64 convolutions of the rows, shared by the children (each is computed once)."""
    with tempfile.TemporaryDirectory() as tmp:
        yield tmp


@pytest.mark.parametrize("env,dtype", cl.JOBS, ids=["%s-%s" % j for j in cl.JOBS])
def test_conv_lattice_is_bit_exact(cuda, cache_dir, env, dtype):
    _run_child(f"_child({env!r}, {dtype!r}, {cache_dir!r})", env)


@pytest.mark.parametrize("family", list(cl.ROUNDING))
def test_conv_rounding_per_element(cuda, family):
    assert K_BAR[family] <= K_DERIVED[family]
    _run_child(f"_child_rounding({family!r})", cl.ROUNDING[family][0])
