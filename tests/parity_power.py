"""What the whole-net parity tests can see.  Every conv kernel is checked by running a U-Net and comparing its logits with the oracle, so a fault
in a layer is found only if it moves the logits by more than the bound.  This module holds

  * CASES: the nets, weights, shapes and plans of tests/test_gpu_deep_levels.py, and ``bound``, the distance that test allows;
  * the standard mutations -- a lost element, a lost column of a slice, a wrong or a stray Dropout2d factor -- planted into one layer's output of the
    oracle (oracle/unet_oracle.py, ``tap``), each returning the largest change of any logit.

tests/test_parity_power_cpu.py asserts that every mutation at every deep layer of every case moves the logits by at least 10 x the bound, and
that on synthetic_state weights the two deepest levels do NOT reach the bound of the tests that use those weights."""
import torch

from oracle import unet_oracle as uo

WIDE = dict(nb_classes=2, in_channels=4, depth=4, start_filters=32, dropout=0.05)
REL_TOL = 2e-5      # of the logit range: the project's bound for weights with BatchNorm gains (golden G18, tests/test_gpu_parity.py)
MASK_P = 0.3        # heavier dropout than the configs', so that the factors matter
DEEP_PIXELS = 48 * 32


def bound(logit_range):
    """The largest |logit - oracle logit| tests/test_gpu_deep_levels.py allows a kernel plan, given max |oracle logit| of the run."""
    return REL_TOL * logit_range


# name -> weights recipe, seed and BatchNorm gain (2.5 unless given), net, input [n, C, H, W], plan options (rcu_unet_options) and the batch prefixes that must give the full run's
# bits.  All full width, depth 4: the smallest shapes that reach the kernels named in ``why``.
CASES = {
    'A': dict(recipe='sensitive_state', seed=21, params=WIDE, shape=(11, 4, 192, 128), prefixes=(3, 9),
              why='24x16 and 12x8 levels; 11 slices = a full eight-slice item + 3 = a full ten-slice fold + 1',
              plans=(dict(), dict(conv_winograd4=2), dict(conv_winograd4=0), dict(conv_winograd=0), dict(conv_winograd4=2, upconv_winograd4=2),
                     dict(act_layout=1), dict(head_winograd4=0))),
    'B': dict(recipe='sensitive_state', seed=22, params=WIDE, shape=(3, 4, 240, 240), prefixes=(2,),
              why='the BraTS slice: levels 60 / 30 / 15 allocated 64 / 32 / 16, stores limited to the real extent',
              plans=(dict(), dict(conv_winograd4=2), dict(pad_levels=0))),
    'C': dict(recipe='sensitive_state', seed=23, params=dict(WIDE, in_channels=3), shape=(2, 3, 192, 256), prefixes=(1,),
              why='the ISIC image: a 24x32 level, a 12x16 bottom level allocated 16x16, three input channels',
              plans=(dict(), dict(conv_winograd4=2))),
    'D': dict(recipe='sensitive_state', seed=24, params=WIDE, shape=(5, 4, 128, 512), prefixes=(3,),
              why='an 8x32 bottom level: the four-slice tile S4T8x32 on a ragged batch',
              plans=(dict(), dict(conv_winograd4=2))),
    'E': dict(recipe='sensitive_state', seed=25, bn_gain=2.0, params=dict(WIDE, residual=True), shape=(2, 4, 192, 128), prefixes=(1,),
              why='residual blocks: the 1x1 conv and the accumulating second unit at the deep levels (BatchNorm gain 2.0: see sensitive_state)',
              plans=(dict(),)),
}


def make_case(name):
    """-> (state, x, masks) of a case: seeded, the same on every machine."""
    case = CASES[name]
    state = getattr(uo, case['recipe'])(case['seed'], bn_gain=case.get('bn_gain', 2.5), **case['params'])
    g = torch.Generator().manual_seed(1000 + case['seed'])
    x = torch.randn(*case['shape'], generator=g)
    _, sites = uo.unet_plan(**case['params'])
    return state, x, uo.sample_masks(sites, case['shape'][0], MASK_P, g)


def layers(params, h, w):
    """[(index, key, height, width, site)] of the tapped layers -- conv units and up-convolutions -- with the extent of their OUTPUT."""
    plan, _ = uo.unet_plan(**params)
    out, level = [], 0
    for op in plan:
        if op['kind'] == 'pool':
            level += 1
        elif op['kind'] == 'up':
            level -= 1
        if op['kind'] in ('unit', 'up'):
            out.append((op['index'], op['key'], h >> level, w >> level, op.get('site')))
    return out


def is_deep(height, width):
    return height * width <= DEEP_PIXELS


class Trace:
    """One slice's forward through the oracle with every tapped layer's output kept, so that a mutated forward recomputes only what lies behind
    the mutated layer (unet_forward's ``tap.resume``)."""

    def __init__(self, state, x, masks, params):
        assert x.shape[0] == 1
        self.state, self.x, self.masks, self.params = state, x, masks, params
        self.outputs = {}
        self.logits = uo.unet_forward(state, x, masks, tap=self._record, **params)
        self.range = float(self.logits.abs().max())

    def _record(self, index, op, tensor):
        self.outputs[index] = tensor
        return tensor

    def response(self, layer, mutate=None, masks=None):
        """max |dlogit| of a forward that is this one up to ``layer``, whose output becomes ``mutate(clone of output)``; ``masks`` (differing from
        the trace's at that layer's site only) are used from ``layer`` on."""
        outputs = self.outputs

        def tap(index, op, tensor):
            return mutate(tensor.clone()) if index == layer and mutate is not None else tensor
        tap.resume = lambda index, op: outputs[index] if index < layer else None
        out = uo.unet_forward(self.state, self.x, self.masks if masks is None else masks, tap=tap, **self.params)
        return float((out - self.logits).abs().max())


def lost_element(trace, layer, far=False):
    """The kernel stored nothing for one element: at the corner pixel (0, 0) -- or (h-1, w-1), where a padded level's real extent ends -- the
    channel with the largest value reads 0."""
    r = -1 if far else 0

    def mutate(t):
        t[0, int(t[0, :, r, r].abs().argmax()), r, r] = 0.0
        return t
    return trace.response(layer, mutate)


def lost_column(trace, layer):
    """The last real column of the slice, every channel, reads 0."""
    def mutate(t):
        t[0, :, :, -1] = 0.0
        return t
    return trace.response(layer, mutate)


def wrong_factor(trace, layer, site):
    """The slice got another slice's Dropout2d factor: the entry of the channel with the largest mean activation flips between 0 and 1 / keep.
    ``trace`` must have run under masks; the layer is recomputed with the changed ``masks`` argument."""
    channel = int(trace.outputs[layer][0].mean((1, 2)).argmax())
    masks = [m.clone() for m in trace.masks]
    masks[site][0, channel] = 0.0 if float(masks[site][0, channel]) != 0.0 else 1.0 / (1.0 - MASK_P)
    return trace.response(layer, None, masks)


def stray_factor(trace, layer):
    """A Dropout2d factor where none belongs: in an eval-mode forward the channel with the largest mean activation is multiplied by 1 / keep."""
    def mutate(t):
        t[0, int(t[0].mean((1, 2)).argmax())] *= 1.0 / (1.0 - MASK_P)
        return t
    return trace.response(layer, mutate)
