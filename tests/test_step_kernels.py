"""The streaming step kernels (csrc/step_kernels.hip: scale, absmax + clamp, the two AdamUniform passes) against the float64
statements of tests/step_oracle.py, with the per-entry bounds stated there.

CPU part (unmarked): the oracle reproduces the reference's golden trajectory; an fp32 numpy emulation of the header's formulae
(separately rounded and with fused multiply-adds) stays inside every bound on every case of the GPU matrix; three emulations
whose maximum overlooks the scalar tail, element 0, or everything past the first grid-stride round leave the parameter bound on
the placements aimed at them while their moments stay inside theirs -- so the bounds admit a correct fp32 implementation and
the placements have teeth.

GPU part: the three C entry points through raw pointers into windows ``buf[k : k + n]`` of buffers of ``n + 16`` floats, so
the test chooses the alignment (4-byte multiples: the kernels' scalar branches), with canaries outside the windows, read-only
arrays compared as a whole and the workspace filled with 0xFF before every call; then the Python optimiser over two
parameters that share one workspace.
"""
import os

import numpy as np
import pytest

import step_oracle as SO

F32 = np.float32
SIZES = (0, 1, 2, 3, 4, 5, 255, 256, 257, 771, 1024, 1025, 4099, 524_288, 524_289, 1_572_871)
SCALE_SIZES = SIZES + (2_097_152, 2_097_157)             # tsamd_scale caps its grid at 2048 workgroups
FULL_MATRIX_MAX = 4099                                   # the full matrix up to here, a reduced set above
STEPS = (1, 7, 1000, 100_000)
LR, B1, B2 = (float(F32(v)) for v in (0.1, 0.9, 0.999))  # what the ABI's `float` arguments hold
# no clamp (checks the maximum of g2) / a clamp that acts (checks the maximum of |g1|) / one that does not (the s <= limit branch)
LIMITS = {"none": -1.0, "clamp": float(F32(0.01)), "loose": 1000.0}
ADAM_ALIGN = ((0, 0, 0, 0), (1, 1, 1, 1), (1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 2, 0), (0, 0, 0, 3))     # floats: p, grad, g1, g2
SCALE_ALIGN = ((0, 0), (1, 1), (0, 1), (1, 0), (3, 2))                                               # floats: in, out
SCALARS = tuple(F32(v) for v in (1.0, 0.37, -2.0, 0.0, np.inf))
G1_SPIKE, G2_SPIKE, GL_SPIKE = -64.0, 4096.0, 50.0
GL_S = float(F32(0.37))


def grid(n, cap=512):
    return max(1, min((n + 1023) // 1024, cap))


def placements(n, reduced=False):
    """Where a maximum hides: first, last, last vector lane, first tail element, lane 63 of wave 0, lane 0 of wave 1, the last
    lane of workgroup 0, the first entry of workgroup 1, the first entry of the second stride round, the middle."""
    full = (0, n - 1, 4 * (n // 4) - 1, 4 * (n // 4), 252, 256, 1020, 1024, 1024 * grid(n), n // 2)
    out = []
    for i in ((0, n - 1, 1024 * grid(n), n // 2) if reduced else full):
        if 0 <= i < n and i not in out:
            out.append(i)
    return out


def spike_pairs(n, reduced=False):
    """(i1, i2): every placement holds the |g1| spike once and the g2 spike once, at different indices where n allows."""
    P = placements(n, reduced)
    return [(P[j], P[(j + 1) % len(P)]) for j in range(len(P))]


def adam_cases(n, modes=tuple(LIMITS)):
    """(i1, i2, mode, step) of the Adam matrix at size n, without the alignments."""
    if n <= FULL_MATRIX_MAX:
        return [(i1, i2, m, t) for (i1, i2) in spike_pairs(n) for m in modes for t in STEPS]
    cases = [(i1, i2, m) for (i1, i2) in spike_pairs(n, True) for m in modes if m != "loose"]
    return [c + (STEPS[j % len(STEPS)],) for j, c in enumerate(cases)]


def adam_base(n):
    """Uniform in [-1, 1], g2 in [0, 1]."""
    rng = np.random.default_rng(1000 + n)
    return {"p": rng.uniform(-1, 1, n).astype(F32), "grad": rng.uniform(-1, 1, n).astype(F32),
            "g1": rng.uniform(-1, 1, n).astype(F32), "g2": rng.uniform(0, 1, n).astype(F32)}


def adam_inputs(base, i1, i2):
    g1, g2 = base["g1"].copy(), base["g2"].copy()
    g1[i1] = G1_SPIKE          # negative: the maximum is of |g1|
    g2[i2] = G2_SPIKE
    return base["p"], base["grad"], g1, g2


def grad_limit_cases(n):
    """(index of the +-50 spike or None, its sign, threshold, all-zero array)."""
    if n <= FULL_MATRIX_MAX:
        cases = [(i, (-1.0, 1.0)[j % 2], thr, False) for j, i in enumerate(placements(n)) for thr in (1.0, GL_SPIKE, 100.0)]
    else:
        cases = [(i, (-1.0, 1.0)[j % 2], thr, False) for j, i in enumerate(placements(n, True)) for thr in (1.0, GL_SPIKE)]
    # no spike: the quiet data clamps against a small threshold and stays below a large one; zeros stay zeros
    return cases + [(None, 1.0, 0.25, False), (None, 1.0, 1.0, False), (None, 1.0, 0.05, True)]


def grad_limit_input(n, idx, sign, zero):
    g = np.zeros(n, F32) if zero else np.random.default_rng(2000 + n).uniform(-1, 1, n).astype(F32)
    if zero and n > 1:
        g[n // 2] = -0.0
    if idx is not None:
        g[idx] = sign * GL_SPIKE
    return g


def scale_input(n):
    """Magnitudes in [2^-10, 1] (no denormal input or product), a +0 and a -0."""
    rng = np.random.default_rng(3000 + n)
    x = (rng.choice((-1.0, 1.0), n) * rng.uniform(2.0 ** -10, 1, n)).astype(F32)
    if n > 2:
        x[n // 3], x[n // 2] = 0.0, -0.0
    return x


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.int32)


def assert_bitwise(got, want, label):
    """Bit for bit, NaN positions instead of NaN payloads."""
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), label
    assert np.array_equal(_bits(got)[~nan], _bits(want)[~nan]), label


def adam_errors(got, ref):
    """Worst error / bound of (p, g1, g2)."""
    out = []
    for g, want, bound in ((got[0], ref.p, SO.param_bound(ref, LR)), (got[1], ref.g1, SO.moment_bound(ref.mag1)),
                           (got[2], ref.g2, SO.moment_bound(ref.mag2))):
        err = np.abs(np.asarray(g, dtype=np.float64) - want)
        assert np.isfinite(err).all()
        out.append(float(np.max(err / np.maximum(bound, 1e-300))) if err.size else 0.0)
    return out


# ---- CPU ----------------------------------------------------------------------------------------------------------------------

def test_oracle_step_matches_reference_trajectory(golden_dir):
    """adam_step, started from zero state, walks the trajectories the reference class itself produced
    (adam_uniform_golden.npz; the bound is test_optimizer.py::test_oracle_matches_reference_trajectory's)."""
    z = np.load(os.path.join(golden_dir, "adam_uniform_golden.npz"))
    for name, values, iters in (("plain", None, None), ("limited", [0.05, 0.01], [3])):
        p = z["p0"].astype(np.float64)
        g1, g2 = np.zeros_like(p), np.zeros_like(p)
        ptr = 0
        for it in range(z[f"{name}_grads"].shape[0]):
            limit = -1.0
            if values is not None:          # the schedule of the reference: the pointer advances after the read
                limit = values[ptr]
                if ptr < len(iters) and it >= iters[ptr]:
                    ptr += 1
            r = SO.adam_step(p, z[f"{name}_grads"][it], g1, g2, 0.2, 0.9, 0.999, it + 1, limit)
            p, g1, g2 = r.p, r.g1, r.g2
            assert np.abs(p - z[f"{name}_traj"][it]).max() <= 1e-14, (name, it)


def test_fp32_emulations_stay_inside_every_bound():
    """Both emulations on every case of the GPU matrix (the alignments do not exist on the host)."""
    worst = np.zeros(3)
    for n in SIZES:
        if n == 0:
            continue
        base = adam_base(n)
        for (i1, i2, mode, step) in adam_cases(n):
            args = adam_inputs(base, i1, i2) + (LR, B1, B2, step, LIMITS[mode])
            ref = SO.adam_step(*args)
            assert ref.clamped == (mode == "clamp"), (n, i1, i2, mode, step)
            for fused in (False, True):
                e = adam_errors(SO.emulate_adam_step(*args, fused=fused), ref)
                assert max(e) <= 1.0, (n, i1, i2, mode, step, fused, e)
                worst = np.maximum(worst, e)
        for (idx, sign, thr, zero) in grad_limit_cases(n):
            g = grad_limit_input(n, idx, sign, zero)
            ref, clamped = SO.grad_limit(g, thr, GL_S)
            got = SO.emulate_grad_limit(g, thr, GL_S)           # (no multiply-add in this one: nothing to fuse)
            if clamped:
                assert np.all(np.abs(got.astype(np.float64) - ref) <= SO.grad_limit_bound(ref)), (n, idx, thr)
            else:
                assert np.array_equal(_bits(got), _bits(g)), (n, idx, thr)
    print("worst error / bound of the emulations (p, g1, g2):", worst)
    # scale: the float64 product of two fp32 values is exact, so its fp32 rounding IS the fp32 product
    for n in (1, 5, 771, 4099):
        x = scale_input(n)
        for s in SCALARS:
            with np.errstate(invalid="ignore", over="ignore"):
                assert_bitwise(SO.emulate_scale(x, s), SO.scale(x, s).astype(F32), (n, s))


def _mutant_placements():
    """(n, seen, target, other): the maximum overlooks ~seen; `target` lies there, `other` does not."""
    for n in (5, 255, 257, 771, 1025, 4099):            # the scalar tail
        for t in dict.fromkeys((4 * (n // 4), n - 1)):
            yield "tail", n, np.arange(n) < 4 * (n // 4), t, 0
    for n in (2, 5, 771, 4099):                         # element 0
        yield "element0", n, np.arange(n) > 0, 0, n - 1
    for n in (524_289, 1_572_871):                      # everything past the first grid-stride round
        yield "stride", n, np.arange(n) < 1024 * grid(n), 1024 * grid(n), 0


def test_mutant_maxima_leave_the_parameter_bound():
    seen_kinds = set()
    for kind, n, seen, target, other in _mutant_placements():
        base = adam_base(n)
        steps = STEPS if n <= FULL_MATRIX_MAX else (7,)
        # a missed g2 spike shows without the clamp, a missed |g1| spike with it (the clamp cancels the denominator)
        for (i1, i2, mode) in ((other, target, "none"), (target, other, "clamp")):
            for step in steps:
                for fused in (False, True):
                    args = adam_inputs(base, i1, i2) + (LR, B1, B2, step, LIMITS[mode])
                    ref = SO.adam_step(*args)
                    e = adam_errors(SO.emulate_adam_step(*args, fused=fused, seen=seen), ref)
                    assert e[0] > 1.0, (kind, n, i1, i2, mode, step, fused, e)
                    assert e[1] <= 1.0 and e[2] <= 1.0, (kind, n, i1, i2, mode, step, fused, e)
                    ok = adam_errors(SO.emulate_adam_step(*args, fused=fused), ref)
                    assert max(ok) <= 1.0, (kind, n, i1, i2, mode, step, fused, ok)
        # the clamp's own maximum: the spike is overlooked, the array stays unclamped
        g = grad_limit_input(n, target, -1.0, False)
        ref, clamped = SO.grad_limit(g, 1.0, GL_S)
        got = SO.emulate_grad_limit(g, 1.0, GL_S, seen=seen)
        assert clamped and not np.all(np.abs(got.astype(np.float64) - ref) <= SO.grad_limit_bound(ref)), (kind, n)
        seen_kinds.add(kind)
    assert seen_kinds == {"tail", "element0", "stride"}


# ---- GPU ----------------------------------------------------------------------------------------------------------------------

CANARY = int(np.array([0xCAFEF00D], dtype=np.uint32).view(np.int32)[0])      # -8.4e6 as a float: would win any maximum here


@pytest.fixture(scope="module")
def gpu():
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from tssplat_amd import _capi
    return torch, _capi.load()


def _stream(torch):
    return int(torch.cuda.current_stream().cuda_stream)


def _window(torch, data, k):
    """A device buffer of n + 16 floats, canaries everywhere but in buf[k : k + n] = data."""
    n = data.numel()
    buf = torch.full((n + 16,), CANARY, dtype=torch.int32, device="cuda").view(torch.float32)
    assert buf.data_ptr() % 16 == 0
    buf[k:k + n] = data
    return buf


def _ptr(buf, k):
    return buf.data_ptr() + 4 * k


def _canaries_intact(rows, k, n):
    """rows: [cases, n + 16] int32 images of buffers after the call."""
    return bool(np.all(rows[:, :k] == CANARY) and np.all(rows[:, k + n:] == CANARY))


def _run_adam(torch, lib, n, cases, aligns):
    """Every case at every alignment on the device, one copy back, then the oracle on the host."""
    base = adam_base(n)
    dev = {k: torch.from_numpy(v).cuda() for k, v in base.items()}
    ws = torch.empty(16, dtype=torch.uint8, device="cuda")
    stream = _stream(torch)
    names = ("p", "g1", "g2")
    out = {k: torch.empty((len(cases) * len(aligns), n + 16), dtype=torch.int32, device="cuda") for k in names}
    r = 0
    for al in aligns:
        win = {k: _window(torch, dev[k], o) for k, o in zip(("p", "grad", "g1", "g2"), al)}
        grad_image = win["grad"].view(torch.int32).clone()
        for (i1, i2, mode, step) in cases:
            p, g1, g2 = win["p"].clone(), win["g1"].clone(), win["g2"].clone()
            assert p.data_ptr() % 16 == 0 and g1.data_ptr() % 16 == 0 and g2.data_ptr() % 16 == 0
            g1[al[2] + i1] = G1_SPIKE
            g2[al[3] + i2] = G2_SPIKE
            ws.fill_(255)                                   # the launch resets its workspace itself
            rc = lib.tsamd_adam_uniform_step(_ptr(p, al[0]), _ptr(win["grad"], al[1]), _ptr(g1, al[2]), _ptr(g2, al[3]), n, LR, B1, B2,
                                             step, LIMITS[mode], ws.data_ptr(), stream)
            assert rc == 0
            for k, b in zip(names, (p, g1, g2)):
                out[k][r].copy_(b.view(torch.int32))
            r += 1
        assert torch.equal(win["grad"].view(torch.int32), grad_image), ("grad was written", n, al)
    host = {k: v.cpu().numpy() for k, v in out.items()}
    refs, worst = {}, np.zeros(3)
    r = 0
    for al in aligns:
        rows = slice(r, r + len(cases))
        for k, o in zip(names, (al[0], al[2], al[3])):
            assert _canaries_intact(host[k][rows], o, n), (k, "written outside its window", n, al)
        for case in cases:
            (i1, i2, mode, step) = case
            if case not in refs:
                refs[case] = SO.adam_step(*adam_inputs(base, i1, i2), LR, B1, B2, step, LIMITS[mode])
                assert refs[case].clamped == (mode == "clamp")
            got = [host[k][r, o:o + n].view(F32) for k, o in zip(names, (al[0], al[2], al[3]))]
            e = adam_errors(got, refs[case])
            assert max(e) <= 1.0, (n, al, case, "error / bound of p, g1, g2", e)
            worst = np.maximum(worst, e)
            r += 1
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(LIMITS))
def test_adam_step_full_matrix(gpu, mode):
    """n <= 4099: every spike pair x every alignment x the four step counts, in one limit mode."""
    torch, lib = gpu
    worst = np.zeros(3)
    for n in SIZES:
        if 0 < n <= FULL_MATRIX_MAX:
            worst = np.maximum(worst, _run_adam(torch, lib, n, adam_cases(n, (mode,)), ADAM_ALIGN))
    print(f"adam {mode}: worst error / bound (p, g1, g2) {worst}")


@pytest.mark.gpu
@pytest.mark.parametrize("n", [n for n in SIZES if n > FULL_MATRIX_MAX])
def test_adam_step_capped_grid(gpu, n):
    """The grid cap exactly, the cap plus one, three stride rounds with a 3-float tail: first, last, first entry of the second
    stride round and the middle, vector and scalar paths, with and without the clamp."""
    torch, lib = gpu
    worst = _run_adam(torch, lib, n, adam_cases(n), (ADAM_ALIGN[0], ADAM_ALIGN[1]))
    print(f"adam n={n}: worst error / bound (p, g1, g2) {worst}")


@pytest.mark.gpu
def test_adam_step_stale_workspace(gpu):
    """A quiet call right after a spiked one, same workspace, nothing reset by the test: the maxima of the first call must
    not leak into the second."""
    torch, lib = gpu
    stream = _stream(torch)
    for n in (771, 4099, 524_289):
        base = adam_base(n)
        ws = torch.empty(16, dtype=torch.uint8, device="cuda")
        ws.fill_(255)
        for mode in ("none", "clamp"):
            spiked = [torch.from_numpy(a.copy()).cuda() for a in adam_inputs(base, n // 2, n - 1)]
            quiet = [torch.from_numpy(base[k].copy()).cuda() for k in ("p", "grad", "g1", "g2")]
            for b in (spiked, quiet):
                assert lib.tsamd_adam_uniform_step(*(t.data_ptr() for t in b), n, LR, B1, B2, 7, LIMITS[mode], ws.data_ptr(), stream) == 0
            ref = SO.adam_step(base["p"], base["grad"], base["g1"], base["g2"], LR, B1, B2, 7, LIMITS[mode])
            e = adam_errors([quiet[j].cpu().numpy() for j in (0, 2, 3)], ref)
            assert max(e) <= 1.0, (n, mode, e)


@pytest.mark.gpu
def test_adam_step_non_finite_gradient(gpu):
    """+inf in grad: every finite entry of p unchanged bit for bit, the inf entry NaN, g1 and g2 inf there.  The kernel's
    arithmetic: both maxima inf, denom = inf, scale = 0, s = inf / inf = NaN fails `s > limit`, p -= 0 * g1.  The reference's
    torch chain gives the same: g1, g2 inf at the entry (utils/optimizer.py:61-62), m2 inf (:68), gr = m1 / (1e-8 + inf) = 0
    at every finite entry and inf / inf = NaN at the entry (:74), s = max|gr| = NaN so `if s > m` is false (:84-85), and
    p.sub_(gr, alpha=lr) leaves the finite entries alone (:88).

    NaN in grad: fmaxf drops NaN from both maxima, so the kernel steps every other entry as if the NaN entry were absent and
    only that entry's p, g1, g2 become NaN.  This DEPARTS from the reference, whose .max() propagates NaN into every entry
    (recorded in include/tssplat_amd.h and DESIGN.md); pinned here against the oracle with the entry masked out of both maxima."""
    torch, lib = gpu
    stream = _stream(torch)
    ws = torch.empty(16, dtype=torch.uint8, device="cuda")
    for n in (5, 771, 1025, 4099):
        base = adam_base(n)
        for al in (ADAM_ALIGN[0], ADAM_ALIGN[1]):
            for bad in dict.fromkeys((0, n - 1, n // 2)):
                i1, i2 = (bad + 1) % n, (bad + 2) % n
                for mode in ("none", "clamp"):
                    for value in (np.inf, np.nan):
                        p0, grad, g1, g2 = (a.copy() for a in adam_inputs(base, i1, i2))
                        grad[bad] = value
                        bufs = [_window(torch, torch.from_numpy(a).cuda(), o) for a, o in zip((p0, grad, g1, g2), al)]
                        grad_image = bufs[1].view(torch.int32).clone()
                        ws.fill_(255)
                        assert lib.tsamd_adam_uniform_step(*(_ptr(b, o) for b, o in zip(bufs, al)), n, LR, B1, B2, 7, LIMITS[mode],
                                                           ws.data_ptr(), stream) == 0
                        assert torch.equal(bufs[1].view(torch.int32), grad_image)
                        rows = [b.view(torch.int32).cpu().numpy()[None] for b in bufs]
                        for j in (0, 2, 3):
                            assert _canaries_intact(rows[j], al[j], n)
                        p, a, b = (rows[j][0, al[j]:al[j] + n].view(F32) for j in (0, 2, 3))
                        label = (n, al, bad, mode, value)
                        keep = np.arange(n) != bad
                        ref = SO.adam_step(p0, grad, g1, g2, LR, B1, B2, 7, LIMITS[mode], mask=keep)
                        if np.isinf(value):
                            assert np.array_equal(_bits(p)[keep], _bits(p0)[keep]), label
                            assert np.isnan(p[bad]) and a[bad] == np.inf and b[bad] == np.inf, label
                        else:
                            assert np.isnan(p[bad]) and np.isnan(a[bad]) and np.isnan(b[bad]), label
                            assert np.all(np.abs(p[keep].astype(np.float64) - ref.p[keep]) <= SO.param_bound(ref, LR)[keep]), label
                        assert np.all(np.abs(a[keep].astype(np.float64) - ref.g1[keep]) <= SO.moment_bound(ref.mag1)[keep]), label
                        assert np.all(np.abs(b[keep].astype(np.float64) - ref.g2[keep]) <= SO.moment_bound(ref.mag2)[keep]), label


def _run_grad_limit(torch, lib, n, offsets):
    cases = grad_limit_cases(n)
    ws = torch.empty(int(lib.tsamd_grad_limit_workspace_bytes()), dtype=torch.uint8, device="cuda")
    stream = _stream(torch)
    out = torch.empty((len(cases) * len(offsets), n + 16), dtype=torch.int32, device="cuda")
    quiet = torch.from_numpy(grad_limit_input(n, None, 1.0, False)).cuda()
    zeros = torch.from_numpy(grad_limit_input(n, None, 1.0, True)).cuda()
    r = 0
    for o in offsets:
        wins = {False: _window(torch, quiet, o), True: _window(torch, zeros, o)}
        for (idx, sign, thr, zero) in cases:
            g = wins[zero].clone()
            assert g.data_ptr() % 16 == 0
            if idx is not None:
                g[o + idx] = sign * GL_SPIKE
            ws.fill_(255)
            assert lib.tsamd_grad_limit(_ptr(g, o), n, thr, GL_S, ws.data_ptr(), stream) == 0
            out[r].copy_(g.view(torch.int32))
            r += 1
    host = out.cpu().numpy()
    r = 0
    for o in offsets:
        assert _canaries_intact(host[r:r + len(cases)], o, n), ("written outside the window", n, o)
        for (idx, sign, thr, zero) in cases:
            g = grad_limit_input(n, idx, sign, zero)
            ref, clamped = SO.grad_limit(g, thr, GL_S)
            got = host[r, o:o + n].view(F32)
            if clamped:
                assert np.all(np.abs(got.astype(np.float64) - ref) <= SO.grad_limit_bound(ref)), (n, o, idx, thr)
            else:
                assert np.array_equal(_bits(got), _bits(g)), (n, o, idx, thr, zero)
            r += 1


@pytest.mark.gpu
def test_grad_limit_matrix(gpu):
    """Above the threshold (3u per entry), at it exactly and below it (bit-identical), all zeros (untouched); every placement
    of the +-50 spike at offsets 0..3 up to n = 4099, the four placements at offsets 0 and 1 above."""
    torch, lib = gpu
    for n in SIZES:
        if n > 0:
            _run_grad_limit(torch, lib, n, (0, 1, 2, 3) if n <= FULL_MATRIX_MAX else (0, 1))


@pytest.mark.gpu
def test_grad_limit_non_finite(gpu):
    """One NaN entry: the clamp is decided by the other entries and the NaN stays NaN.  One +inf entry: every finite entry
    becomes +-0 (s / inf = 0) and the inf entry NaN."""
    torch, lib = gpu
    ws = torch.empty(int(lib.tsamd_grad_limit_workspace_bytes()), dtype=torch.uint8, device="cuda")
    stream = _stream(torch)
    for n in (5, 771, 4099):
        for o in (0, 3):
            for bad in dict.fromkeys((0, n - 1, n // 2)):
                keep = np.arange(n) != bad
                for value, spike, thr in ((np.nan, (bad + 1) % n, 1.0), (np.nan, None, 2.0), (np.inf, None, 1.0)):
                    g = grad_limit_input(n, spike, -1.0, False)
                    g[bad] = value
                    buf = _window(torch, torch.from_numpy(g).cuda(), o)
                    ws.fill_(255)
                    assert lib.tsamd_grad_limit(_ptr(buf, o), n, thr, GL_S, ws.data_ptr(), stream) == 0
                    row = buf.view(torch.int32).cpu().numpy()[None]
                    assert _canaries_intact(row, o, n)
                    got = row[0, o:o + n].view(F32)
                    label = (n, o, bad, value, spike)
                    if np.isinf(value):
                        assert np.isnan(got[bad]) and np.all(got[keep] == 0), label
                        assert np.array_equal(np.signbit(got[keep]), np.signbit(g[keep])), label      # GL_S > 0
                        continue
                    ref, clamped = SO.grad_limit(g, thr, GL_S, mask=keep)
                    assert clamped == (spike is not None), label
                    if clamped:
                        assert np.isnan(got[bad]), label
                        assert np.all(np.abs(got[keep].astype(np.float64) - ref[keep]) <= SO.grad_limit_bound(ref)[keep]), label
                    else:
                        assert np.array_equal(_bits(got), _bits(g)), label


def _run_scale(torch, lib, n, cases):
    """cases: (in offset, out offset, in place, scalar)."""
    x = scale_input(n)
    xd = torch.from_numpy(x).cuda()
    stream = _stream(torch)
    out = torch.empty((len(cases), n + 16), dtype=torch.int32, device="cuda")
    for r, (ki, ko, inplace, s) in enumerate(cases):
        src = _window(torch, xd, ki)
        dst = src if inplace else torch.full((n + 16,), CANARY, dtype=torch.int32, device="cuda").view(torch.float32)
        assert src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0
        image = src.view(torch.int32).clone()
        sd = torch.tensor([float(s)], dtype=torch.float32, device="cuda")
        assert lib.tsamd_scale(_ptr(src, ki), sd.data_ptr(), _ptr(dst, ko), n, stream) == 0
        if not inplace:
            assert torch.equal(src.view(torch.int32), image), ("in was written", n, ki, ko, s)
        out[r].copy_(dst.view(torch.int32))
    host = out.cpu().numpy()
    for r, (ki, ko, inplace, s) in enumerate(cases):
        label = (n, ki, ko, inplace, float(s))
        assert _canaries_intact(host[r:r + 1], ko, n), label
        got = host[r, ko:ko + n].view(F32)
        with np.errstate(invalid="ignore", over="ignore"):
            assert_bitwise(got, x * s, label)
        if s == 1:                       # out of place: an exact copy; in place: left alone
            assert np.array_equal(_bits(got), _bits(x)), label


@pytest.mark.gpu
def test_scale_matrix(gpu):
    """out = in * scalar, bit for bit against the fp32 product (NaN positions and the sign of zero included): in place and out
    of place, aligned, misaligned and mixed, tail-only to four stride rounds of the 2048-workgroup grid."""
    torch, lib = gpu
    for n in SCALE_SIZES:
        if n == 0:
            continue
        if n <= FULL_MATRIX_MAX:
            cases = [(ki, ko, False, s) for (ki, ko) in SCALE_ALIGN for s in SCALARS] + [(k, k, True, s) for k in (0, 1, 2, 3) for s in SCALARS]
        else:
            cases = [(ki, ko, False, s) for (ki, ko) in ((0, 0), (3, 2)) for s in SCALARS[:2]] + [(k, k, True, s) for k in (0, 1) for s in SCALARS[:2]]
        _run_scale(torch, lib, n, cases)


@pytest.mark.gpu
def test_empty_arrays_touch_nothing(gpu):
    """n = 0 returns TSAMD_OK and writes nothing -- not the arrays, not the workspace -- with live and with null pointers."""
    torch, lib = gpu
    stream = _stream(torch)
    bufs = [torch.full((16,), CANARY, dtype=torch.int32, device="cuda") for _ in range(4)]
    ws = torch.full((16,), 255, dtype=torch.uint8, device="cuda")
    sd = torch.tensor([0.37], dtype=torch.float32, device="cuda")
    p, g, a, b = (t.data_ptr() for t in bufs)
    for k in (0, 4):
        assert lib.tsamd_adam_uniform_step(p + k, g + k, a + k, b + k, 0, LR, B1, B2, 1, LIMITS["clamp"], ws.data_ptr(), stream) == 0
        assert lib.tsamd_grad_limit(p + k, 0, 1.0, GL_S, ws.data_ptr(), stream) == 0
        assert lib.tsamd_scale(p + k, sd.data_ptr(), g + k, 0, stream) == 0
        assert lib.tsamd_scale(p + k, sd.data_ptr(), p + k, 0, stream) == 0
    assert lib.tsamd_adam_uniform_step(None, None, None, None, 0, LR, B1, B2, 1, -1.0, None, stream) == 0
    assert lib.tsamd_grad_limit(None, 0, 1.0, GL_S, None, stream) == 0
    assert lib.tsamd_scale(None, None, None, 0, stream) == 0
    torch.cuda.synchronize()
    assert all(bool((t == CANARY).all()) for t in bufs) and bool((ws == 255).all()) and float(sd) == float(F32(0.37))


@pytest.mark.gpu
def test_optimizer_two_parameters_one_workspace(gpu):
    """AdamUniform over two parameters of one group: [257, 3] with gradients of order 1 and [5, 3] with gradients of order
    1e3, the second a contiguous view one float into a larger tensor (p misaligned, the zeros_like states aligned).  Before
    each of four steps the state is read from the device and the oracle takes the same single step: the maxima are per
    parameter (the large one must not scale the small one, the shared workspace is reset between the two launches) and the
    limit schedule -- the reference's, whose counter runs per parameter, utils/optimizer.py:76-89 -- reaches the kernel."""
    torch, lib = gpu
    from tssplat_amd.utils import AdamUniform
    rng = np.random.default_rng(7)
    pa = torch.nn.Parameter(torch.from_numpy(rng.uniform(-1, 1, (257, 3)).astype(F32)).cuda())
    store = torch.zeros(32, dtype=torch.float32, device="cuda")
    store[1:16] = torch.from_numpy(rng.uniform(-1, 1, 15).astype(F32)).cuda()
    pb = torch.nn.Parameter(store[1:16].view(5, 3))
    assert store.data_ptr() % 16 == 0 and pb.data_ptr() % 16 == 4 and pb.is_contiguous()
    values, iters = [0.05, 0.01], [2]
    opt = AdamUniform([pa, pb], lr=0.1, grad_limit=True, grad_limit_values=values, grad_limit_iters=iters)
    cc = ptr = 0
    limits_seen = []
    for it in range(4):
        grads = [rng.uniform(-1, 1, (257, 3)).astype(F32), (1e3 * rng.uniform(-1, 1, (5, 3))).astype(F32)]
        before = []
        for q, g in zip((pa, pb), grads):
            st = opt.state[q]
            before.append([q.detach().cpu().numpy().copy()] + [st[k].cpu().numpy().copy() if k in st else np.zeros(q.shape, F32) for k in ("g1", "g2")])
            q.grad = torch.from_numpy(g).cuda()
        opt.step()
        for q, g, (p0, a0, b0) in zip((pa, pb), grads, before):
            limit = values[ptr]                                  # the reference's schedule, once per parameter
            if ptr < len(iters) and cc >= iters[ptr]:
                ptr += 1
            cc += 1
            limits_seen.append(limit)
            ref = SO.adam_step(p0, g, a0, b0, LR, B1, B2, it + 1, float(F32(limit)))
            st = opt.state[q]
            assert st["step"] == it + 1 and st["g1"].data_ptr() % 16 == 0 and st["g2"].data_ptr() % 16 == 0
            e = adam_errors([q.detach().cpu().numpy(), st["g1"].cpu().numpy(), st["g2"].cpu().numpy()], ref)
            assert max(e) <= 1.0, (it, tuple(q.shape), limit, e)
    assert limits_seen == [0.05, 0.05, 0.05, 0.01, 0.01, 0.01, 0.01, 0.01] and opt.cc == 8
    assert float(store[0]) == 0.0 and float(store[16:].abs().sum()) == 0.0         # nothing written around the view
