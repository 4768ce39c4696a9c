"""The per-launch kernel-node updates of the library's HIP graphs (csrc/eval_launch.cpp: eval_graph_launch, train_loop_launch).

A graph's nodes keep pointers to argument blocks the launch layer owns; a launch rewrites what changed -- coefficients, the
order, the gradient's address, the energy copy's, the optimiser's scalars -- and hands the node its parameter block again.
Driven through the C ABI on the smallest scene with shared vertices (two tiles per sphere, so both the tile node and the
finish node carry arguments that change) and compared with stream launches of the same kernels on the same inputs: bit for bit."""
import ctypes as C

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


class Flags:
    smooth_eng_coeff = 2e-4
    barrier_coeff = 2e-4
    increase_order_iter = 1000


@pytest.fixture(scope="module")
def scene():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from tssplat_amd import scenes
    from tssplat_amd.energies import SmoothnessBarrierEnergy
    sc = scenes.make_scene("kuhn8", 2)
    mod = SmoothnessBarrierEnergy(sc.rest, sc.tets, Flags)
    info = mod.tet_sp.plan_info()
    assert info["n_tiles"] >= 2 and info["finish_vertices"] > 0, info      # shared vertices: the finish kernel sums staged rows
    x0 = torch.from_numpy(scenes.deform(sc, 0.3)).cuda()
    return mod.tet_sp, x0, mod                                              # (mod keeps the handle alive)


def test_eval_graph_launch_updates_coefficients_gradient_address_and_energy_copy(scene):
    from tssplat_amd import _capi, tet_spheres_ext
    lib = _capi.load()
    ts, x0, _ = scene
    h, stream = ts._handle(), tet_spheres_ext._stream_ptr(x0.device)
    x = x0.clone()
    scale = torch.full((1,), 0.75, dtype=torch.float32, device=x.device)
    order = 2

    def eager(c1, c2):
        e, g = torch.zeros((), device=x.device), torch.zeros_like(x)
        _capi.check(lib.tsamd_forward_backward(h, x.data_ptr(), scale.data_ptr(), c1, c2, order, stream, e.data_ptr(), g.data_ptr()))
        return float(e), ts.energy_terms(), g

    e_g, g_own, g_other = torch.zeros((), device=x.device), torch.zeros_like(x), torch.zeros_like(x)
    e_copy = torch.zeros(1, device=x.device)
    graph = C.c_void_p()
    _capi.check(lib.tsamd_graph_create(h, x.data_ptr(), scale.data_ptr(), order, e_g.data_ptr(), g_own.data_ptr(), C.byref(graph)))
    try:
        def replay(c1, c2, copy=None, grad=None):
            for t in (g_own, g_other):
                t.fill_(-7.0)                      # (what a launch does not write stays -7)
            e_g.fill_(-7.0)
            e_copy.fill_(-7.0)
            if copy is None and grad is None:
                _capi.check(lib.tsamd_graph_launch(graph, c1, c2, stream))
            else:
                _capi.check(lib.tsamd_graph_launch_to(graph, c1, c2, stream, None if copy is None else copy.data_ptr(),
                                                      None if grad is None else grad.data_ptr()))
            return float(e_g), ts.energy_terms(), g_own.clone(), g_other.clone(), float(e_copy)

        untouched = torch.full_like(x, -7.0)
        first, second = (2e-4, 2e-4), (0.5e-4, 3e-4)
        # 1: the coefficients the graph was not created with
        e, terms, own, other, copy = replay(*first)
        e_ref, terms_ref, g_ref = eager(*first)
        assert (e, terms) == (e_ref, terms_ref) and torch.equal(own, g_ref)
        assert torch.equal(other, untouched) and copy == -7.0
        assert float(g_ref.abs().max()) > 0 and e_ref > 0                  # (the deformation inverts no tet: terms[1] may be 0)
        # 2: another pair
        e, terms, own, other, copy = replay(*second)
        e_ref2, terms_ref2, g_ref2 = eager(*second)
        assert (e, terms) == (e_ref2, terms_ref2) and torch.equal(own, g_ref2)
        assert e_ref2 != e_ref and not torch.equal(g_ref2, g_ref)           # (the update was needed)
        # 3: same coefficients, another gradient buffer and an energy-copy destination
        e, terms, own, other, copy = replay(*second, copy=e_copy, grad=g_other)
        assert (e, terms) == (e_ref2, terms_ref2) and torch.equal(other, g_ref2)
        assert torch.equal(own, untouched) and copy == e_ref2
        # ... and back: the graph's own buffer, no copy, the first pair again
        e, terms, own, other, copy = replay(*first)
        assert (e, terms) == (e_ref, terms_ref) and torch.equal(own, g_ref)
        assert torch.equal(other, untouched) and copy == -7.0
    finally:
        lib.tsamd_graph_destroy(graph)


def test_train_loop_launch_updates_order_limit_and_coefficients(scene):
    from tssplat_amd import _capi, tet_spheres_ext
    lib = _capi.load()
    ts, x0, _ = scene
    h, stream = ts._handle(), tet_spheres_ext._stream_ptr(x0.device)
    n, lr, b1, b2 = 3, 0.05, 0.9, 0.999
    # two launches of three steps: every per-step argument differs between them (and between the steps of the second)
    schedule = [dict(c1=[2e-4] * 3, c2=[2e-4] * 3, order=[2, 2, 2], limit=[-1.0, -1.0, -1.0]),
                dict(c1=[1e-4, 1.5e-4, 3e-4], c2=[3e-4, 2.5e-4, 1e-4], order=[4, 2, 4], limit=[0.01, -1.0, 0.004])]

    # eager: the same kernels from the stream, one step at a time
    xe = x0.clone()
    g1e, g2e, grad = torch.zeros_like(xe), torch.zeros_like(xe), torch.zeros_like(xe)
    ws = torch.zeros(16, dtype=torch.uint8, device=xe.device)
    e = torch.zeros((), device=xe.device)
    energies_e, step = [], 0
    for launch in schedule:
        for k in range(n):
            step += 1
            _capi.check(lib.tsamd_forward_backward(h, xe.data_ptr(), None, launch["c1"][k], launch["c2"][k], launch["order"][k], stream,
                                                   e.data_ptr(), grad.data_ptr()))
            _capi.check(lib.tsamd_adam_uniform_step(xe.data_ptr(), grad.data_ptr(), g1e.data_ptr(), g2e.data_ptr(), xe.numel(), lr, b1, b2, step,
                                                    launch["limit"][k], ws.data_ptr(), stream))
            energies_e.append(float(e))

    xf = x0.clone()
    g1f, g2f, gradf = torch.zeros_like(xf), torch.zeros_like(xf), torch.zeros_like(xf)
    ring = torch.zeros(n, dtype=torch.float32, device=xf.device)
    wsf = torch.zeros(int(lib.tsamd_train_loop_workspace_bytes(n)), dtype=torch.uint8, device=xf.device)
    loop = C.c_void_p()
    _capi.check(lib.tsamd_train_loop_create(h, xf.data_ptr(), gradf.data_ptr(), g1f.data_ptr(), g2f.data_ptr(), ring.data_ptr(), wsf.data_ptr(), n,
                                            C.byref(loop)))
    try:
        energies_f = []
        for i, launch in enumerate(schedule):
            _capi.check(lib.tsamd_train_loop_launch(loop, (C.c_float * n)(*launch["c1"]), (C.c_float * n)(*launch["c2"]),
                                                    (C.c_int32 * n)(*launch["order"]), lr, b1, b2, 1 + n * i, (C.c_float * n)(*launch["limit"]), stream))
            energies_f += ring.cpu().tolist()
    finally:
        lib.tsamd_train_loop_destroy(loop)
    assert energies_f == energies_e
    assert torch.equal(xf, xe) and torch.equal(g1f, g1e) and torch.equal(g2f, g2e)
    assert len(set(energies_e)) == 2 * n and float((xe - x0).abs().max()) > 1e-3        # (every step did something else)
