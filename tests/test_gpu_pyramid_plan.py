"""The Gaussian pyramid's launch list as the library ran it (SiftContext.pyramid_plan(), the
planner of csrc/sift_pyramid_plan.h): under each forcing hook the plan holds the kind of launch
that the hook forces, so the bit-identity tests of test_gpu_gauss.py, which compare every such
variant's levels with one level per launch, did run the kernel they name; and the number of kernel
launches the launchers report lies between the entry count and that count plus the entries that
may take two launches.

The tile-duo hook (tiles always + duo always) asks for tile duos only when every level can be tiled;
3 x 203x97 u8 (rows 203 bytes apart) cannot tile level 0, so there the plan must hold what the two
flags force separately (tiles and paired levels), and tile duos at the other two shapes."""
import numpy as np
import pytest

import sgpu
from sgpu_types import default_options
from sift_synth import synth_batch

pytestmark = pytest.mark.gpu

C = sgpu.SiftContext
DUO, DUO_OFF, TILE = C.DEBUG_DUO_ALWAYS, C.DEBUG_DUO_OFF, C.DEBUG_GAUSS_TILE_ALWAYS
MULTI_LEVEL = {"duo", "trio", "tile_duo", "tile_duo_one"}
ONE_OR_TWO_LAUNCHES = {"two", "tile_two", "tile_duo_one"}
N_LEVELS = {"level": 1, "tile": 1, "two": 2, "tile_two": 2, "tile_duo": 2, "tile_duo_one": 3,
            "duo": 2, "trio": 3}

# (name, debug flags, (trio, pairs), kinds of which the plan must hold one / None: no multi-level kind)
HOOKS = [
    ("shipped", 0, (C.TRIO_OFF, C.PAIRS_END), set()),
    ("duo always, pairs from the end", DUO, (C.TRIO_OFF, C.PAIRS_END), {"duo"}),
    ("duo always, pairs from the front", DUO, (C.TRIO_OFF, C.PAIRS_FRONT), {"duo"}),
    ("tiles always", TILE, (C.TRIO_OFF, C.PAIRS_END), {"tile", "tile_two"}),
    ("tile duo", TILE | DUO, (C.TRIO_OFF, C.PAIRS_END), {"tile_duo", "tile_duo_one"}),
    ("duo off", DUO_OFF, (C.TRIO_OFF, C.PAIRS_END), None),
]
TRIO_HOOK = ("trio always", 0, (C.TRIO_ALWAYS, C.PAIRS_END), {"trio"})


@pytest.mark.parametrize("n,w,h", [(2, 16, 16), (3, 203, 97), (1, 104, 33)])
def test_forced_kernels_are_in_the_plan(gpu_ctx, n, w, h):
    imgs = synth_batch(n, w, h, 200 + w % 13)
    gpu_ctx.set_options(default_options())
    # the three-level kernel where test_trio_levels_equal_single_level shows fewer launches
    hooks = HOOKS + ([TRIO_HOOK] if (n, w, h) == (3, 203, 97) else [])
    all_tiled = False
    try:
        for name, flags, schedule, forced in hooks:
            gpu_ctx.set_schedule(*schedule)
            gpu_ctx.set_debug_flags(flags)
            gpu_ctx.extract(imgs)
            plan = gpu_ctx.pyramid_plan()
            launches, filters = gpu_ctx.pyramid_launches()
            kinds = [k for k, _ in plan]
            if name == "tiles always":
                all_tiled = set(kinds) <= {"tile", "tile_two"}
            if forced is None:
                assert not MULTI_LEVEL & set(kinds), (name, plan)
            elif name == "tile duo" and not all_tiled:
                # the hook takes the tile-duo schedule only when every level can be tiled (a u8
                # image whose rows are no multiple of 4 bytes apart: level 0 cannot); otherwise
                # its two flags force what each forces alone
                assert "duo" in kinds and "tile" in kinds, (name, plan)
            else:
                assert not forced or forced & set(kinds), (name, plan)
            assert all(len(levels) == N_LEVELS[k] for k, levels in plan), (name, plan)
            covered = [lv for _, levels in plan for lv in levels]
            assert len(covered) == len(set(covered)) == filters, (name, plan)
            two = sum(k in ONE_OR_TWO_LAUNCHES for k in kinds)
            assert len(plan) <= launches <= len(plan) + two, (name, launches, plan)
    finally:
        gpu_ctx.set_schedule()
        gpu_ctx.set_debug_flags(0)


def test_pyramid_plan_needs_an_extract():
    ctx = sgpu.SiftContext(0, default_options())
    try:
        assert sgpu.lib().sgpu_debug_pyramid_plan(ctx._ctx, None, 0) == sgpu.SGPU_EINVAL
        with pytest.raises(RuntimeError):
            ctx.pyramid_plan()
        ctx.extract(np.zeros((16, 16), np.uint8))
        out = np.full(7, -7, np.int32)   # room for one entry: one is written, all are counted
        assert sgpu.lib().sgpu_debug_pyramid_plan(ctx._ctx, out.ctypes.data, 7) == len(ctx.pyramid_plan())
        assert out[0] >= 0 and tuple(out[1:3]) == (0, 0)
    finally:
        ctx.close()
