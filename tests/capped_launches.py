"""The launches that cap their grid and let each wave or workgroup walk the remaining work in a loop, and the shapes at which
tests/test_gpu_capped_launches.py runs them: one row per kernel, the cap as literals, the shape, and the arithmetic that makes the shape a
test of the loop -- a third trip exists (the prefetch / ping-pong / barrier of the loop has been through both of its states), the last item is
partial, and items straddle image boundaries.  tests/test_capped_launches_cpu.py reads every cap from the kernel sources and re-derives every
number below: whoever moves a cap learns that the shapes must move too.  Nothing here needs a device or the package."""
import collections

Row = collections.namedtuple('Row', 'kernel source walkers item n_images hw work items third_trips last_item one_image_items')
# walkers          waves (PostNet, density energy, head stream), workgroups (temperature) or threads (quantile apply) of a capped launch
# item             voxels (elements) one walker takes per trip
# work             voxels (elements) of the call = n_images * hw
# items            ceil(work / item)
# third_trips      walkers that take a third item: items - 2 * walkers
# last_item        voxels (elements) in the last item: 1 .. item - 1, i.e. partial
# one_image_items  items of a single image: <= walkers, so a one-image call is a one-trip call (the pieces of assertion (b))

POSTNET_SHAPE = (3, 457, 401)          # hw = 183,257 = 32 * 5726 + 25; also the density energy's voxel count
HEAD_SHAPE = (5, 508, 516)             # HW = 262,128 = 64 * 4095 + 48
HEAD_MODEL = dict(in_channels=2, depth=2, start_filters=32)
TEMPERATURE_SHAPE = (3, 340 * 301)     # hw = 102,340 = 64 * 1599 + 4
QUANTILE_N16 = 4300003                 # the 16-byte form: 1,075,000 quads + a 3-element tail
QUANTILE_N4 = 1100003                  # the element-by-element form

POSTNET_WGS, POSTNET_WAVES, POSTNET_GROUP = 2048, 4, 32
HEAD_WGS_PER_CU, HEAD_CUS, HEAD_THREADS, HEAD_GROUP = 8, 256, 256, 64
TN_MAX_GROUPS, TN_TILE, TN_STAGE_MAX = 2048, 64, 256
QA_MAX_GROUPS, QA_THREADS = 2048, 256


def _row(kernel, source, walkers, item, n_images, hw):
    work = n_images * hw
    items = -(-work // item)
    return Row(kernel, source, walkers, item, n_images, hw, work, items, max(0, items - 2 * walkers), work - (items - 1) * item, -(-hw // item))


ROWS = {
    'postnet': _row('postnet_kernel<1,2,3>', 'rcu_postnet.hip', POSTNET_WGS * POSTNET_WAVES, POSTNET_GROUP, 3, 457 * 401),
    'density_energy': _row('density_energy_kernel<1,2>', 'rcu_density.hip', POSTNET_WGS * POSTNET_WAVES, POSTNET_GROUP, 3, 457 * 401),
    'head_stream': _row('head_stream_kernel<C,SIG>, head_stream_sample_kernel<C>', 'rcu_pointwise.hip',
                        HEAD_CUS * HEAD_WGS_PER_CU * (HEAD_THREADS // 64), HEAD_GROUP, 5, 508 * 516),
    'temperature': _row('temperature_nll_kernel<STAGED,...>', 'rcu_temperature.hip', TN_MAX_GROUPS, TN_TILE, 3, 340 * 301),
    'quantile_apply_16': _row('quantile_apply_kernel (16-byte form)', 'rcu_quantile.hip', QA_MAX_GROUPS * QA_THREADS, 4, 1, QUANTILE_N16),
    'quantile_apply_4': _row('quantile_apply_kernel (scalar form)', 'rcu_quantile.hip', QA_MAX_GROUPS * QA_THREADS, 1, 1, QUANTILE_N4),
}

# the same numbers written out by hand ("Capped launches"); test_capped_launches_cpu.py holds ROWS to them
STATED = {
    'postnet': dict(hw=183257, hw_mod=25, work=549771, items=17181, walkers=8192, third_trips=797, last_item=11),
    'density_energy': dict(hw=183257, hw_mod=25, work=549771, items=17181, walkers=8192, third_trips=797, last_item=11),
    'head_stream': dict(hw=262128, hw_mod=48, work=1310640, items=20479, walkers=8192, third_trips=4095, last_item=48),
    'temperature': dict(hw=102340, hw_mod=4, work=307020, items=4798, walkers=2048, third_trips=702, last_item=12),
}

# PostNet above the cap: (channels, classes, nb_convs); the last is the largest LDS image rcu_postnet_create accepts (4 x 37,632 B)
POSTNET_CASES = ((32, 2, 3), (64, 3, 3), (96, 4, 3))
POSTNET_P = 0.3
# density energy above the cap: (F, K, pitch)
DENSITY_CASES = ((32, 2, 32), (45, 3, 48), (64, 2, 64))
# temperature above the cap: (P, C)
TEMPERATURE_CASES = ((3, 2), (2, 3))
TEMPERATURE_CANDIDATES = (0, 48, 96)
# the unstaged temperature form (tests/test_gpu_temperature.py): P * (C - 1) = 259 > TN_STAGE_MAX
UNSTAGED_CASES = ((37, 8), (257, 2))


def postnet_capped_case(channels, classes, nb_convs, masked):
    """(state, x [3, C, 457, 401] float32, masks or None) of one PostNet case above the cap; seeded by the case alone."""
    import torch

    import postnet_reference as pr
    from oracle import unet_oracle as uo
    n, h, w = POSTNET_SHAPE
    state = uo.postnet_synthetic_state(channels + classes, channels, classes, nb_convs)
    x = pr.features(n, channels, h, w, channels)
    masks = pr.draw_masks(n, channels, nb_convs, POSTNET_P, torch.Generator().manual_seed(7 * channels)) if masked else None
    return state, x, masks
