"""The conv lattice (tests/conv_lattice.py) on the CPU: the reference alone satisfies the exactness conditions the GPU
test's bit-for-bit equality rests on, the epilogues exercise clamp, both lrelu sides and 16-bit rounding, and the case
table still reaches every launch-plan instance (asked of the library's own planner, one child process per knob
environment: the knobs are read once per process)."""
import functools
import json
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

import conv_lattice as cl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def _acc(rid):
    return cl.conv_acc(rid)


def _exact_in(t, dtype):
    return torch.equal(t.to(dtype).to(t.dtype), t)


@pytest.mark.parametrize("rid", list(cl.ROWS))
def test_lattice_is_exact(rid):
    """Operands are integers of the stated range, stored exactly in f32, bf16 and f16; every partial sum is bounded by
    8 K (Winograd: 48 * 3 * cin_p per transformed accumulator, from integer U and V) < 2^24; an f32 conv of the
    lattice equals the fp64 one; every epilogue value survives the round trip through f32."""
    r = cl.ROWS[rid]
    x, w = cl.operands(rid)
    wmax = 4 if rid in cl.WINO else 2
    assert torch.equal(x, x.round()) and x.abs().max() <= 4 and torch.equal(w, w.round()) and w.abs().max() <= wmax
    assert x.abs().max() == 4 and w.abs().max() == wmax   # the whole range is used
    for dt in (torch.bfloat16, torch.float16):
        assert _exact_in(x, dt) and _exact_in(w, dt)
    assert not x[..., r.cin:].any() and not w[..., r.cin:].any() and not w[r.cout_valid:].any()
    K = r.k * r.k * r.cin_p
    acc = _acc(rid)
    if rid in cl.WINO:
        assert torch.equal(w, (w / 2).round() * 2)   # even
        wd = w.double().permute(0, 3, 1, 2)
        u = torch.einsum("uk,ocyk->ocyu", cl.G_MAT, wd)
        assert torch.equal(u, u.round()) and u.abs().max() <= 6 and _exact_in(u, torch.float16)
        xp = F.pad(x.double().permute(0, 3, 1, 2), (r.pad, r.pad + 2, r.pad, r.pad))
        for nu in range(4):
            v = F.conv2d(xp.reshape(-1, 1, *xp.shape[2:]), cl.BT_MAT[nu].reshape(1, 1, 1, 4), stride=(1, 2))
            assert torch.equal(v, v.round()) and v.abs().max() <= 8 and _exact_in(v, torch.float16)
            kern = u.abs()[..., nu, None] * cl.BT_MAT[nu].abs()
            m_abs = F.conv2d(xp.abs(), kern, stride=(1, 2))   # >= any partial sum of the nu-th accumulator
            assert m_abs.max() <= 48 * 3 * r.cin_p <= 147456
        assert 3 * 147456 < 2 ** 24
        assert acc.abs().max() <= 16 * K
    else:
        assert K <= 9 * 1024 and 8 * K <= 73728 < 2 ** 24
        assert acc.abs().max() <= 8 * K
    acc32 = F.conv2d(x.permute(0, 3, 1, 2), w.permute(0, 3, 1, 2), padding=r.pad).permute(0, 2, 3, 1)
    assert torch.equal(acc32.double(), acc)
    assert not acc[..., r.cout_valid:].any()
    for epi in cl.EPILOGUES:
        osc, bias = cl.epilogue_params(rid, epi, acc)
        ref = cl.apply_epilogue(acc, epi, osc, bias)
        assert torch.equal(ref.float().double(), ref), epi
        if osc is not None:   # the intermediate acc * oscale + bias too (exact with or without FMA contraction)
            pre = acc * osc.double()[:, None, None, :]
            assert torch.equal(pre.float().double(), pre)
            assert osc.shape == (r.n, r.cout_p) and bias.shape == (r.cout_p,)
            assert r.n == 1 or not torch.equal(osc[0], osc[1])   # the exponents differ between samples


@pytest.mark.parametrize("rid", list(cl.ROWS))
def test_act_epilogue_shares(rid):
    """Per row, on the valid channels of the `act` reference: >= 2 % clamped, >= 20 % negative, >= 20 % positive and
    unclamped."""
    r = cl.ROWS[rid]
    acc = _acc(rid)
    osc, bias = cl.epilogue_params(rid, "act", acc)
    ref = cl.apply_epilogue(acc, "act", osc, bias)[..., :r.cout_valid]
    top = cl.EPILOGUES["act"]["clamp"] * cl.EPILOGUES["act"]["out_mul"]
    clamped = (ref.abs() == top).double().mean().item()
    neg = (ref < 0).double().mean().item()
    pos = ((ref > 0) & (ref < top)).double().mean().item()
    print(f"[conv-lattice shares] {rid}: clamped {clamped:.3f}, negative {neg:.3f}, positive unclamped {pos:.3f}")
    assert clamped >= 0.02 and neg >= 0.20 and pos >= 0.20, (clamped, neg, pos)


def test_linear_epilogue_exercises_16_bit_rounding():
    """For each 16-bit output type, at least 5 % of the elements of the `linear` cases stored in that type (the rows whose
    variants pair `linear` with it; valid channels) are not representable in it, so a store that truncates instead of
    rounding to nearest even cannot pass.  bf16 holds 8 bits: 26 %.  f16 holds every m / 8 below 256, so only sums with
    |acc| > 256 * 2^e count: 0 % for K < 512, 7 % at the deepest direct K, more on the Winograd rows (even weights up to
    4); the table reaches the share through its deep rows."""
    pairs = sorted({(rid, odt) for env, dtype in cl.JOBS for rid in cl.PLAN[env]
                    for epi, odt, _ in cl.variants(rid, dtype) if epi == "linear" and odt in (cl.BF16, cl.F16)})
    assert {p[1] for p in pairs} == {cl.BF16, cl.F16}
    total, inexact = {cl.BF16: 0, cl.F16: 0}, {cl.BF16: 0, cl.F16: 0}
    for rid, odt in pairs:
        r = cl.ROWS[rid]
        acc = _acc(rid)
        osc, bias = cl.epilogue_params(rid, "linear", acc)
        ref = cl.apply_epilogue(acc, "linear", osc, bias)[..., :r.cout_valid].float()
        total[odt] += ref.numel()
        inexact[odt] += int((ref.to(cl.OUT_TORCH[odt]).float() != ref).sum())
    share = {odt: inexact[odt] / total[odt] for odt in total}
    print(f"[conv-lattice shares] linear, not representable: bf16 {share[cl.BF16]:.4f}, f16 {share[cl.F16]:.4f}")
    assert all(v >= 0.05 for v in share.values()), share


@pytest.mark.parametrize("env", [e for e in cl.ENVS if any(
    epi == "linear" and odt in (cl.BF16, cl.F16) for d in cl.dtypes_of(e) for rid in cl.PLAN[e]
    for epi, odt, _ in cl.variants(rid, d))])
def test_a_truncating_store_cannot_pass_in_any_environment(env):
    """The pooled share above says little about one kernel family: most f16-inexact `linear` values come from the deep
    Winograd row.  So per knob environment (one kernel family or forced tile each) and per 16-bit output type, the
    `linear` values its rows store in that type hold at least 1000 elements that round-to-nearest-even moves AWAY from
    zero (valid channels).  A store that truncates instead changes every one of them, so it fails the equality in
    that environment whatever the other families do; 1000 rather than 1 so that no single row or channel carries it.
    The direct kernels get them from their deep-K rows (s3c, s3d, p1k; hg4: its 256- to 512-channel rows); the halo
    direct conv (K <= 864) has none in f16 and stores `linear` as bf16 only, where every row must have them."""
    count = {cl.BF16: 0, cl.F16: 0}
    per_row = {}
    for rid, odt in sorted({(rid, odt) for d in cl.dtypes_of(env) for rid in cl.PLAN[env]
                            for epi, odt, _ in cl.variants(rid, d) if epi == "linear" and odt in count}):
        r = cl.ROWS[rid]
        acc = _acc(rid)
        osc, bias = cl.epilogue_params(rid, "linear", acc)
        ref = cl.apply_epilogue(acc, "linear", osc, bias)[..., :r.cout_valid].float()
        away = int((ref.to(cl.OUT_TORCH[odt]).float().abs() > ref.abs()).sum())
        count[odt] += away
        per_row[rid, odt] = away
    print(f"[conv-lattice shares] {env}: linear values rounded away from zero: bf16 {count[cl.BF16]}, f16 {count[cl.F16]}")
    assert all(v >= 1000 for v in count.values()), count
    for rid in cl.HCONV:
        if (rid, cl.BF16) in per_row:
            assert per_row[rid, cl.BF16] >= 1000, (rid, per_row[rid, cl.BF16])
            assert (rid, cl.F16) not in per_row


def test_variants_cover_every_combination():
    """Every instance of the table sees the three epilogues, the four output types and the three layouts (ToRGB: its
    NCHW f32 output with the three epilogues; the four large rows run `act` to NHWC only and share their instances'
    epilogue code with the small rows of the same kernels); each combination is one conv_check_call accepts."""
    seen = {}
    for env, dtype in cl.JOBS:
        for rid in cl.PLAN[env]:
            vs = cl.variants(rid, dtype)
            assert vs[0][0] == "act" and (rid in cl.TORGB or vs[0][1:] == (cl.DTYPE_CODE[dtype], cl.NHWC))
            for epi, odt, lay in vs:
                assert lay != cl.NCHW or odt == cl.F32
            seen.setdefault(cl.plan_name(env, rid, dtype), set()).update(vs)
    for name, vs in seen.items():
        if name.startswith("torgb"):
            assert {v[0] for v in vs} == set(cl.EPILOGUES)
            continue
        if all(name != cl.plan_name(e, rid, d) or rid in cl.LARGE for e, d in cl.JOBS for rid in cl.PLAN[e]):
            continue   # an instance only the large rows reach
        assert {v[0] for v in vs} == set(cl.EPILOGUES), name
        assert {v[1] for v in vs} == {cl.F32, cl.BF16, cl.F16, cl.F16_IEEE}, name
        assert {v[2] for v in vs} == {cl.NHWC, cl.NCHW, cl.NHWC16}, name


def _ask_planner(env):
    """{dtype: {row id: plan name}} for the rows of `env`, from the library's planner in a child process."""
    code = (f"import sys, json; sys.path.insert(0, {ROOT!r}); sys.path.insert(0, {os.path.join(ROOT, 'tests')!r})\n"
            "import conv_lattice as cl\n"
            "from image_compression_2_amd import _native as nv\n"
            f"env = {env!r}\n"
            "out = {}\n"
            "for dt in cl.dtypes_of(env):\n"
            "    for rid in cl.PLAN[env]:\n"
            "        r = cl.ROWS[rid]\n"
            "        if rid in cl.WINO:\n"
            "            name = nv.wino_plan(r.n, r.h, r.w, r.cin_p, r.cout_p, r.pad)\n"
            "        else:\n"
            "            name = nv.conv_plan(*cl.plan_query(rid, dt))\n"
            "        out.setdefault(dt, {})[rid] = name\n"
            "print(json.dumps(out))\n")
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, IC2_DEV="1", **cl.ENVS[env]),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-4000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.fixture(scope="module")
def planned():
    return {env: _ask_planner(env) for env in cl.ENVS}


@pytest.mark.parametrize("env", list(cl.ENVS))
def test_each_row_runs_the_instance_it_declares(planned, env):
    """Fails when a planner change silently moves a row to another kernel."""
    for dt, names in planned[env].items():
        for rid, name in names.items():
            assert name == cl.plan_name(env, rid, dt), (env, dt, rid, name)


def test_table_reaches_every_plan_name(planned):
    """The names the rows return are exactly the names ic2_conv_plan can return for bf16, f16 and f32 operands (the
    eight tile stems, split-K of tiles 0-5 and of the 256 x 256 8-phase tile, its tail split, the 256 + 128 two-launch
    form, six hg4, six hconv, ToRGB, and the f16 twin of every 16-bit one), and the Winograd rows cover row-blocked and
    flat tiles."""
    direct, wino = set(), set()
    for env, per_dt in planned.items():
        for names in per_dt.values():
            (wino if env.startswith("wino") else direct).update(names.values())
    print(f"[conv-lattice reach] {len(direct)} direct-conv plan names: {sorted(direct)}")
    print(f"[conv-lattice reach] Winograd plan names: {sorted(wino)}")
    assert sorted(direct) == cl.ALL_DIRECT_NAMES
    assert any(n.endswith("w_f16") for n in wino) and any(not n.endswith("w_f16") for n in wino)
    # short K: K / 32 in {1, 2, 3, 5} on every 4-stage tile (and the 2-stage f32 tile), K / 64 in {1, 2, 3} on both
    # 8-phase tiles
    for t in range(1, 6):
        ks = {cl.ROWS[rid].cin_p // 32 for rid in cl.PLAN["tile%d" % t] if cl.ROWS[rid].k == 1}
        assert {1, 2, 3, 5} <= ks, (t, ks)
    assert {1, 2, 3, 5} <= {cl.ROWS[rid].cin_p // 32 for rid in cl.PLAN["f32"] if cl.ROWS[rid].k == 1}
    for t in (6, 7):
        ks = {cl.ROWS[rid].cin_p // 64 for rid in cl.PLAN["tile%d" % t] if cl.ROWS[rid].k == 1}
        assert {1, 2, 3} <= ks, (t, ks)
    # geometry edges
    rows = cl.ROWS.values()
    assert any(r.h != r.w for r in rows) and {0, 1, 2} <= {r.pad for r in rows}
    assert any(r.n >= 2 and ((r.h + 2 * r.pad - r.k + 1) * (r.w + 2 * r.pad - r.k + 1)) % 16 for r in rows)
    assert any(r.h == 2 and r.w == 2 for r in rows) and any(r.h == 1 for r in rows)
    assert any(r.cout_valid < r.cout_p for r in rows)
