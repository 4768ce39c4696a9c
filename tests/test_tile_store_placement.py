"""Where the gradient tile kernels store to global memory, read off the gfx950 code object the library was built with (no GPU needed).

A tile's passes are separated by workgroup barriers and every phase is as long as its slowest wave.  A global store issued in
front of a barrier costs more than its issue slot: the `vmcnt` counter retires in order, so the next wait of that wave for
an OLDER load -- the compiler places a full `s_waitcnt vmcnt(0)` at the head of pass 3 -- also waits for the store's
acknowledgement, and the workgroup's other waves wait for that wave at the next barrier.  The per-tile energy pair used to be
stored right behind the H-store barrier (tile_kernel.hip: kSumLate); it is now the last wave's last instruction.  The property
asserted here is the general one: in every tile kernel built with the gradient, no `global_store*` instruction stands in front
of the kernel's last `s_barrier` (the one between the scatter and the per-vertex sums).  The body is straight-line code from
barrier to barrier, so the order of addresses is the order of execution."""
import os
import sys

import pytest

from tssplat_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

LLVM = "/opt/rocm/lib/llvm/bin"


@pytest.mark.skipif(not all(os.path.exists(os.path.join(LLVM, t)) for t in ("llvm-objdump", "llvm-readelf", "llvm-objcopy", "clang-offload-bundler")),
                    reason="needs the ROCm LLVM tools")
def test_no_global_store_in_front_of_the_last_barrier_of_a_gradient_tile_kernel():
    import kernel_metadata
    _capi.load()
    code = kernel_metadata.kernel_instructions(_capi.lib_path(), "tile_")
    grad = {k: v for k, v in code.items() if ("tile_energy_kernelILb1E" in k or "tile_shared_index_kernelILb1E" in k)}
    # with the gradient: built-in / explicit operator / rebuild_dminv in the default layout, for plans with and without shared
    # index planes, and the three fat-wave layouts
    assert len(grad) == 9, sorted(grad)
    for name, ops in grad.items():
        barriers = [i for i, op in enumerate(ops) if op == "s_barrier"]
        stores = [i for i, op in enumerate(ops) if op.startswith("global_store")]
        assert len(barriers) >= 6, (name, len(barriers))          # the six barriers of a tile (tile_kernel.hip: tile_body)
        assert stores, name                                        # the vertex sums and the energy pair
        assert not any(op.startswith(("flat_store", "buffer_store", "scratch_store")) for op in ops), name   # (stores come in one flavour)
        early = [i for i in stores if i < barriers[-1]]
        assert not early, f"{name}: {len(early)} global store(s) in front of the last barrier (instruction {early[0]} of {len(ops)}, barrier at {barriers[-1]})"
