"""The solver's packed pointing cache (``PackCache`` / ``PackedPointing``) and launch context (``FusedContext`` /
``ObsPass``) on the host: every device call, allocation and release they issue, against a fake ``capi``
(tests/packed_pointing_case.py).  No GPU, no native library.

The expected logs below (``PACKS``, ``ROUTES``) are literals.  They were recorded by playing the very same scenarios
against the routines these types replaced, as they stood in the commit before: ``SolverLHS._pack_pass`` and
``_pack_pass_otf`` (with ``release_packed``), ``SolverLHS._fused_first_half`` / ``_fused_second_half`` on the dictionary
context, and the launch loop of ``SolverRHS._exec_fused``, all under the same fake -- never by running the code under
test.  That context was on the fly or not as a whole, so the three route passes went through it as [packed, arrays]
and [on the fly]; the recorded calls stand here in pass order.  Device addresses read "b<k>+<offset>": the k-th
``device_malloc`` of the scenario.  5 detectors x 2**26 samples make the on-the-fly fill work in batches of 2, 2 and 1
(nothing is really allocated)."""

import pytest

import packed_pointing_case as case
from toast_amd import capi
from toast_amd.ops import packed_pointing
from toast_amd.ops.mapmaker_solve import SolverLHS
from toast_amd.ops.packed_pointing import FusedContext, ObsPass, PackedPointing


class Api:
    """The scenarios' steps on the code under test."""

    def operator(self, packed_pointing):
        op = SolverLHS(name="lhs", packed_pointing=packed_pointing)
        op._fused_plan = dict(key=None, generation=0)
        return op

    def pack_cached(self, op, c, p, in_solve):
        cache = op._pack_cache()
        return None if cache is None else cache.cached(FusedContext(**c), ObsPass(**p), in_solve)

    def pack_otf(self, op, c, p, in_solve):
        cache = op._pack_cache()
        if cache is None:
            return None
        s = case.OTF_SOURCE
        return cache.on_the_fly(FusedContext(**c), ObsPass(**p), in_solve, (id(self), s["nside"], s["nest"]),
                                case.descriptor, s["n_submap"])

    def fields(self, pk):
        return None if pk is None else (pk.key, pk.qu, pk.cal, pk.corr, pk.pair, list(pk.blocks))

    def bytes_per_sample(self, pk):
        return None if pk is None else pk.bytes_per_sample

    def release(self, op):
        op.release_packed()
        return "_fused_plan" not in op.__dict__

    @staticmethod
    def context(c, passes):
        ctx = FusedContext(passes=[], **c)
        for p in passes:
            p = dict(p)
            if p.get("pk") is not None:
                pk = PackedPointing()
                pk.key, pk.qu, pk.cal, pk.corr, pk.pair, pk.blocks = p["pk"]
                p["pk"] = pk
            ctx.passes.append(ObsPass(**p))
        return ctx

    def first_half(self, c, passes):
        SolverLHS._fused_first_half(self.context(c, passes))

    def second_half(self, c, passes):
        SolverLHS._fused_second_half(self.context(c, passes))

    def rhs_loop(self, c, passes):
        ctx = self.context(c, passes)
        for ps, p in zip(ctx.passes, passes):
            ctx.scan_project_signal(ps, *case.signal_rows(p))


@pytest.fixture
def install(monkeypatch):
    def put(fake):
        for name, value in fake.install().items():
            monkeypatch.setattr(capi, name, value)

    return put


PACKS = {
    'cached_TTT': dict(
        result={'key': 'b0', 'qu': 'b1', 'cal': 'b2', 'corr': 'b3', 'pair': True, 'blocks': [('b0', 160), ('b1', 640),
            ('b2', 40), ('b3', 192)]},
        log=[
            ('malloc', 160, -2),
            ('malloc', 640, -2),
            ('malloc', 40, -2),
            ('malloc', 192, -2),
            ('offset_pack_pointing_onepass', 66304, 512, (0, 1, 2, 3, 4), 131328, (1, 2, 3, 4, 5), 131584,
             (0, 1, 2, 3, 4), 131840, 8, 17, 132096, 8, 34, (4, 3, 2, 1, 0), 132352, 8, 68, 8, ((0, 7),),
             'b0', 'b1', 'b2', 'b3'),
        ],
        bytes=14,
        plan_dropped=True,
        release_log=[
            ('release', 'b0', 160),
            ('release', 'b1', 640),
            ('release', 'b2', 40),
            ('release', 'b3', 192),
        ],
    ),
    'cached_TTF': dict(
        result={'key': 'b0', 'qu': 'b1', 'cal': 'b2', 'corr': 0, 'pair': True, 'blocks': [('b0', 160), ('b1', 640),
            ('b2', 40)]},
        log=[
            ('malloc', 160, -2),
            ('malloc', 640, -2),
            ('malloc', 40, -2),
            ('malloc', 192, -2),
            ('offset_pack_pointing_onepass', 66304, 512, (0, 1, 2, 3, 4), 131328, (1, 2, 3, 4, 5), 131584,
             (0, 1, 2, 3, 4), 131840, 8, 17, 132096, 8, 34, (4, 3, 2, 1, 0), 132352, 8, 68, 8, ((0, 7),),
             'b0', 'b1', 'b2', 'b3'),
            ('release', 'b3', 192),
        ],
        bytes=18,
        plan_dropped=True,
        release_log=[
            ('release', 'b0', 160),
            ('release', 'b1', 640),
            ('release', 'b2', 40),
        ],
    ),
    'cached_TFF': dict(
        result={'key': 'b0', 'qu': 'b1', 'cal': 'b2', 'corr': 0, 'pair': False, 'blocks': [('b0', 160), ('b1', 640),
            ('b2', 40)]},
        log=[
            ('malloc', 160, -2),
            ('malloc', 640, -2),
            ('malloc', 40, -2),
            ('malloc', 192, -2),
            ('offset_pack_pointing_onepass', 66304, 512, (0, 1, 2, 3, 4), 131328, (1, 2, 3, 4, 5), 131584,
             (0, 1, 2, 3, 4), 131840, 8, 17, 132096, 8, 34, (4, 3, 2, 1, 0), 132352, 8, 68, 8, ((0, 7),),
             'b0', 'b1', 'b2', 'b3'),
            ('release', 'b3', 192),
        ],
        bytes=20,
        plan_dropped=True,
        release_log=[
            ('release', 'b0', 160),
            ('release', 'b1', 640),
            ('release', 'b2', 40),
        ],
    ),
    'cached_F': dict(
        result=None,
        log=[
            ('malloc', 160, -2),
            ('malloc', 640, -2),
            ('malloc', 40, -2),
            ('malloc', 192, -2),
            ('offset_pack_pointing_onepass', 66304, 512, (0, 1, 2, 3, 4), 131328, (1, 2, 3, 4, 5), 131584,
             (0, 1, 2, 3, 4), 131840, 8, 17, 132096, 8, 34, (4, 3, 2, 1, 0), 132352, 8, 68, 8, ((0, 7),),
             'b0', 'b1', 'b2', 'b3'),
            ('release', 'b3', 192),
            ('release', 'b0', 160),
            ('release', 'b1', 640),
            ('release', 'b2', 40),
        ],
        bytes=None,
        plan_dropped=False,
        release_log=[],
    ),
    'cached_no_pair_sum_block_weights_accepted': dict(
        result={'key': 'b0', 'qu': 'b1', 'cal': 'b2', 'corr': 'b4', 'pair': True, 'blocks': [('b0', 160), ('b1', 640),
            ('b2', 40), ('b4', 192)]},
        log=[
            ('malloc', 160, -2),
            ('malloc', 640, -2),
            ('malloc', 40, -2),
            ('malloc_fails', 192, -2),
            ('offset_pack_pointing', 66304, 512, (0, 1, 2, 3, 4), 131328, (1, 2, 3, 4, 5), 131584, (0, 1, 2,
             3, 4), 131840, 8, 17, 132096, 8, 34, (4, 3, 2, 1, 0), 132352, 8, 68, 8, ((0, 7),), 'b0', 'b1',
             'b2'),
            ('malloc', 192, -2),
            ('offset_pack_pair_weights', 'b1', 'b4', 5, 8, ((0, 7),)),
        ],
        bytes=14,
        plan_dropped=True,
        release_log=[
            ('release', 'b0', 160),
            ('release', 'b1', 640),
            ('release', 'b2', 40),
            ('release', 'b4', 192),
        ],
    ),
    'cached_no_pair_sum_block_weights_refused': dict(
        result={'key': 'b0', 'qu': 'b1', 'cal': 'b2', 'corr': 0, 'pair': True, 'blocks': [('b0', 160), ('b1', 640),
            ('b2', 40)]},
        log=[
            ('malloc', 160, -2),
            ('malloc', 640, -2),
            ('malloc', 40, -2),
            ('malloc_fails', 192, -2),
            ('offset_pack_pointing', 66304, 512, (0, 1, 2, 3, 4), 131328, (1, 2, 3, 4, 5), 131584, (0, 1, 2,
             3, 4), 131840, 8, 17, 132096, 8, 34, (4, 3, 2, 1, 0), 132352, 8, 68, 8, ((0, 7),), 'b0', 'b1',
             'b2'),
            ('malloc', 192, -2),
            ('offset_pack_pair_weights', 'b1', 'b4', 5, 8, ((0, 7),)),
            ('release', 'b4', 192),
        ],
        bytes=18,
        plan_dropped=True,
        release_log=[
            ('release', 'b0', 160),
            ('release', 'b1', 640),
            ('release', 'b2', 40),
        ],
    ),
    'cached_onepass_off': dict(
        result={'key': 'b0', 'qu': 'b1', 'cal': 'b2', 'corr': 'b3', 'pair': True, 'blocks': [('b0', 160), ('b1', 640),
            ('b2', 40), ('b3', 192)]},
        log=[
            ('malloc', 160, -2),
            ('malloc', 640, -2),
            ('malloc', 40, -2),
            ('offset_pack_pointing', 66304, 512, (0, 1, 2, 3, 4), 131328, (1, 2, 3, 4, 5), 131584, (0, 1, 2,
             3, 4), 131840, 8, 17, 132096, 8, 34, (4, 3, 2, 1, 0), 132352, 8, 68, 8, ((0, 7),), 'b0', 'b1',
             'b2'),
            ('malloc', 192, -2),
            ('offset_pack_pair_weights', 'b1', 'b3', 5, 8, ((0, 7),)),
        ],
        bytes=14,
        plan_dropped=True,
        release_log=[
            ('release', 'b0', 160),
            ('release', 'b1', 640),
            ('release', 'b2', 40),
            ('release', 'b3', 192),
        ],
    ),
    'cached_pair_weights_off': dict(
        result={'key': 'b0', 'qu': 'b1', 'cal': 'b2', 'corr': 0, 'pair': True, 'blocks': [('b0', 160), ('b1', 640),
            ('b2', 40)]},
        log=[
            ('malloc', 160, -2),
            ('malloc', 640, -2),
            ('malloc', 40, -2),
            ('offset_pack_pointing', 66304, 512, (0, 1, 2, 3, 4), 131328, (1, 2, 3, 4, 5), 131584, (0, 1, 2,
             3, 4), 131840, 8, 17, 132096, 8, 34, (4, 3, 2, 1, 0), 132352, 8, 68, 8, ((0, 7),), 'b0', 'b1',
             'b2'),
        ],
        bytes=18,
        plan_dropped=True,
        release_log=[
            ('release', 'b0', 160),
            ('release', 'b1', 640),
            ('release', 'b2', 40),
        ],
    ),
    'cached_second_block_fails': dict(
        result=None,
        log=[
            ('malloc', 160, -2),
            ('malloc_fails', 640, -2),
            ('release', 'b0', 160),
        ],
        bytes=None,
        plan_dropped=False,
        release_log=[],
    ),
    'cached_no_room': dict(
        result=None,
        log=[],
        bytes=None,
        plan_dropped=False,
        release_log=[],
    ),
    'cached_just_room': dict(
        result={'key': 'b0', 'qu': 'b1', 'cal': 'b2', 'corr': 'b3', 'pair': True, 'blocks': [('b0', 160), ('b1', 640),
            ('b2', 40), ('b3', 192)]},
        log=[
            ('malloc', 160, -2),
            ('malloc', 640, -2),
            ('malloc', 40, -2),
            ('malloc', 192, -2),
            ('offset_pack_pointing_onepass', 66304, 512, (0, 1, 2, 3, 4), 131328, (1, 2, 3, 4, 5), 131584,
             (0, 1, 2, 3, 4), 131840, 8, 17, 132096, 8, 34, (4, 3, 2, 1, 0), 132352, 8, 68, 8, ((0, 7),),
             'b0', 'b1', 'b2', 'b3'),
        ],
        bytes=14,
        plan_dropped=True,
        release_log=[
            ('release', 'b0', 160),
            ('release', 'b1', 640),
            ('release', 'b2', 40),
            ('release', 'b3', 192),
        ],
    ),
    'guard_odd_n_samp': dict(
        result=None,
        log=[],
        bytes=None,
        plan_dropped=False,
        release_log=[],
    ),
    'guard_nnz_1': dict(
        result=None,
        log=[],
        bytes=None,
        plan_dropped=False,
        release_log=[],
    ),
    'guard_no_detectors': dict(
        result=None,
        log=[],
        bytes=None,
        plan_dropped=False,
        release_log=[],
    ),
    'guard_outside_a_solve': dict(
        result=None,
        log=[],
        bytes=None,
        plan_dropped=False,
        release_log=[],
    ),
    'guard_env_off': dict(
        result=None,
        log=[],
        bytes=None,
        plan_dropped=False,
        release_log=[],
    ),
    'guard_trait_off': dict(
        result=None,
        log=[],
        bytes=None,
        plan_dropped=False,
        release_log=[],
    ),
    'cached_same_identity': dict(
        result={'key': 'b0', 'qu': 'b1', 'cal': 'b2', 'corr': 'b3', 'pair': True, 'blocks': [('b0', 160), ('b1', 640),
            ('b2', 40), ('b3', 192)]},
        log=[
            ('malloc', 160, -2),
            ('malloc', 640, -2),
            ('malloc', 40, -2),
            ('malloc', 192, -2),
            ('offset_pack_pointing_onepass', 66304, 512, (0, 1, 2, 3, 4), 131328, (1, 2, 3, 4, 5), 131584,
             (0, 1, 2, 3, 4), 131840, 8, 17, 132096, 8, 34, (4, 3, 2, 1, 0), 132352, 8, 68, 8, ((0, 7),),
             'b0', 'b1', 'b2', 'b3'),
        ],
        bytes=14,
        again_same_object=True,
        again_result={'key': 'b0', 'qu': 'b1', 'cal': 'b2', 'corr': 'b3', 'pair': True, 'blocks': [('b0', 160), ('b1', 640),
            ('b2', 40), ('b3', 192)]},
        again_log=[],
        plan_dropped=True,
        release_log=[
            ('release', 'b0', 160),
            ('release', 'b1', 640),
            ('release', 'b2', 40),
            ('release', 'b3', 192),
        ],
    ),
    'cached_changed_identity': dict(
        result={'key': 'b0', 'qu': 'b1', 'cal': 'b2', 'corr': 'b3', 'pair': True, 'blocks': [('b0', 160), ('b1', 640),
            ('b2', 40), ('b3', 192)]},
        log=[
            ('malloc', 160, -2),
            ('malloc', 640, -2),
            ('malloc', 40, -2),
            ('malloc', 192, -2),
            ('offset_pack_pointing_onepass', 66304, 512, (0, 1, 2, 3, 4), 131328, (1, 2, 3, 4, 5), 131584,
             (0, 1, 2, 3, 4), 131840, 8, 17, 132096, 8, 34, (4, 3, 2, 1, 0), 132352, 8, 68, 8, ((0, 7),),
             'b0', 'b1', 'b2', 'b3'),
        ],
        bytes=14,
        again_same_object=False,
        again_result={'key': 'b4', 'qu': 'b5', 'cal': 'b6', 'corr': 'b7', 'pair': True, 'blocks': [('b4', 160), ('b5', 640),
            ('b6', 40), ('b7', 192)]},
        again_log=[
            ('release', 'b0', 160),
            ('release', 'b1', 640),
            ('release', 'b2', 40),
            ('release', 'b3', 192),
            ('malloc', 160, -2),
            ('malloc', 640, -2),
            ('malloc', 40, -2),
            ('malloc', 192, -2),
            ('offset_pack_pointing_onepass', 66304, 512, (0, 1, 2, 3, 4), 131336, (1, 2, 3, 4, 5), 131584,
             (0, 1, 2, 3, 4), 131840, 8, 17, 132096, 8, 34, (4, 3, 2, 1, 0), 132352, 8, 68, 8, ((0, 7),),
             'b4', 'b5', 'b6', 'b7'),
        ],
        plan_dropped=True,
        release_log=[
            ('release', 'b4', 160),
            ('release', 'b5', 640),
            ('release', 'b6', 40),
            ('release', 'b7', 192),
        ],
    ),
    'otf_TTT': dict(
        result={'key': 'b0', 'qu': 'b1', 'cal': 'b2', 'corr': 'b6', 'pair': True, 'blocks': [('b0', 1342177280), ('b1',
            5368709120), ('b2', 40), ('b6', 1610612736)]},
        log=[
            ('malloc', 1342177280, -2),
            ('malloc', 5368709120, -2),
            ('malloc', 40, -2),
            ('malloc', 1073741824, -2),
            ('malloc', 3221225472, -2),
            ('malloc', 16, -2),
            ('malloc', 1610612736, -2),
            ('otf_pixels_healpix', ('pt', 'd0', 'd1'), (0, 1), 'b3', 67108864, ((0, 67108863),), 'b5', 12,
             512),
            ('otf_stokes_weights', ('pt', 'd0', 'd1'), (0, 1), 'b4', 67108864, ((0, 67108863),)),
            ('offset_pack_pointing_onepass', 66304, 512, (0, 1), 'b3', (0, 1), 'b4', (0, 1), 131840,
             67108864, 17, 132096, 67108864, 34, (4, 3), 132352, 67108864, 68, 67108864, ((0, 67108863),),
             'b0', 'b1', 'b2', 'b6'),
            ('otf_pixels_healpix', ('pt', 'd2', 'd3'), (0, 1), 'b3', 67108864, ((0, 67108863),), 'b5', 12,
             512),
            ('otf_stokes_weights', ('pt', 'd2', 'd3'), (0, 1), 'b4', 67108864, ((0, 67108863),)),
            ('offset_pack_pointing_onepass', 66304, 512, (0, 1), 'b3', (0, 1), 'b4', (2, 3), 131840,
             67108864, 17, 132096, 67108864, 34, (2, 1), 132352, 67108864, 68, 67108864, ((0, 67108863),),
             'b0+536870912', 'b1+2147483648', 'b2+16', 'b6+536870912'),
            ('otf_pixels_healpix', ('pt', 'd4'), (0,), 'b3', 67108864, ((0, 67108863),), 'b5', 12, 512),
            ('otf_stokes_weights', ('pt', 'd4'), (0,), 'b4', 67108864, ((0, 67108863),)),
            ('offset_pack_pointing_onepass', 66304, 512, (0,), 'b3', (0,), 'b4', (4,), 131840, 67108864, 17,
             132096, 67108864, 34, (0,), 132352, 67108864, 68, 67108864, ((0, 67108863),), 'b0+1073741824',
             'b1+4294967296', 'b2+32', 'b6+1073741824'),
            ('release', 'b3', 1073741824),
            ('release', 'b4', 3221225472),
            ('release', 'b5', 16),
        ],
        bytes=14,
        plan_dropped=True,
        release_log=[
            ('release', 'b0', 1342177280),
            ('release', 'b1', 5368709120),
            ('release', 'b2', 40),
            ('release', 'b6', 1610612736),
        ],
    ),
    'otf_second_batch_without_pair_words': dict(
        result={'key': 'b0', 'qu': 'b1', 'cal': 'b2', 'corr': 'b7', 'pair': True, 'blocks': [('b0', 1342177280), ('b1',
            5368709120), ('b2', 40), ('b7', 1610612736)]},
        log=[
            ('malloc', 1342177280, -2),
            ('malloc', 5368709120, -2),
            ('malloc', 40, -2),
            ('malloc', 1073741824, -2),
            ('malloc', 3221225472, -2),
            ('malloc', 16, -2),
            ('malloc', 1610612736, -2),
            ('otf_pixels_healpix', ('pt', 'd0', 'd1'), (0, 1), 'b3', 67108864, ((0, 67108863),), 'b5', 12,
             512),
            ('otf_stokes_weights', ('pt', 'd0', 'd1'), (0, 1), 'b4', 67108864, ((0, 67108863),)),
            ('offset_pack_pointing_onepass', 66304, 512, (0, 1), 'b3', (0, 1), 'b4', (0, 1), 131840,
             67108864, 17, 132096, 67108864, 34, (4, 3), 132352, 67108864, 68, 67108864, ((0, 67108863),),
             'b0', 'b1', 'b2', 'b6'),
            ('otf_pixels_healpix', ('pt', 'd2', 'd3'), (0, 1), 'b3', 67108864, ((0, 67108863),), 'b5', 12,
             512),
            ('otf_stokes_weights', ('pt', 'd2', 'd3'), (0, 1), 'b4', 67108864, ((0, 67108863),)),
            ('offset_pack_pointing_onepass', 66304, 512, (0, 1), 'b3', (0, 1), 'b4', (2, 3), 131840,
             67108864, 17, 132096, 67108864, 34, (2, 1), 132352, 67108864, 68, 67108864, ((0, 67108863),),
             'b0+536870912', 'b1+2147483648', 'b2+16', 'b6+536870912'),
            ('otf_pixels_healpix', ('pt', 'd0', 'd1'), (0, 1), 'b3', 67108864, ((0, 67108863),), 'b5', 12,
             512),
            ('otf_stokes_weights', ('pt', 'd0', 'd1'), (0, 1), 'b4', 67108864, ((0, 67108863),)),
            ('offset_pack_pointing', 66304, 512, (0, 1), 'b3', (0, 1), 'b4', (0, 1), 131840, 67108864, 17,
             132096, 67108864, 34, (4, 3), 132352, 67108864, 68, 67108864, ((0, 67108863),), 'b0', 'b1',
             'b2', ('pair_words', False)),
            ('otf_pixels_healpix', ('pt', 'd2', 'd3'), (0, 1), 'b3', 67108864, ((0, 67108863),), 'b5', 12,
             512),
            ('otf_stokes_weights', ('pt', 'd2', 'd3'), (0, 1), 'b4', 67108864, ((0, 67108863),)),
            ('offset_pack_pointing', 66304, 512, (0, 1), 'b3', (0, 1), 'b4', (2, 3), 131840, 67108864, 17,
             132096, 67108864, 34, (2, 1), 132352, 67108864, 68, 67108864, ((0, 67108863),), 'b0+536870912',
             'b1+2147483648', 'b2+16', ('pair_words', False)),
            ('otf_pixels_healpix', ('pt', 'd4'), (0,), 'b3', 67108864, ((0, 67108863),), 'b5', 12, 512),
            ('otf_stokes_weights', ('pt', 'd4'), (0,), 'b4', 67108864, ((0, 67108863),)),
            ('offset_pack_pointing', 66304, 512, (0,), 'b3', (0,), 'b4', (4,), 131840, 67108864, 17, 132096,
             67108864, 34, (0,), 132352, 67108864, 68, 67108864, ((0, 67108863),), 'b0+1073741824',
             'b1+4294967296', 'b2+32', ('pair_words', False)),
            ('offset_pack_pairs', 'b0', 5, 67108864, ((0, 67108863),)),
            ('release', 'b3', 1073741824),
            ('release', 'b4', 3221225472),
            ('release', 'b5', 16),
            ('release', 'b6', 1610612736),
            ('malloc', 1610612736, -2),
            ('offset_pack_pair_weights', 'b1', 'b7', 5, 67108864, ((0, 67108863),)),
        ],
        bytes=14,
        plan_dropped=True,
        release_log=[
            ('release', 'b0', 1342177280),
            ('release', 'b1', 5368709120),
            ('release', 'b2', 40),
            ('release', 'b7', 1610612736),
        ],
    ),
    'otf_second_batch_not_ok': dict(
        result=None,
        log=[
            ('malloc', 1342177280, -2),
            ('malloc', 5368709120, -2),
            ('malloc', 40, -2),
            ('malloc', 1073741824, -2),
            ('malloc', 3221225472, -2),
            ('malloc', 16, -2),
            ('malloc', 1610612736, -2),
            ('otf_pixels_healpix', ('pt', 'd0', 'd1'), (0, 1), 'b3', 67108864, ((0, 67108863),), 'b5', 12,
             512),
            ('otf_stokes_weights', ('pt', 'd0', 'd1'), (0, 1), 'b4', 67108864, ((0, 67108863),)),
            ('offset_pack_pointing_onepass', 66304, 512, (0, 1), 'b3', (0, 1), 'b4', (0, 1), 131840,
             67108864, 17, 132096, 67108864, 34, (4, 3), 132352, 67108864, 68, 67108864, ((0, 67108863),),
             'b0', 'b1', 'b2', 'b6'),
            ('otf_pixels_healpix', ('pt', 'd2', 'd3'), (0, 1), 'b3', 67108864, ((0, 67108863),), 'b5', 12,
             512),
            ('otf_stokes_weights', ('pt', 'd2', 'd3'), (0, 1), 'b4', 67108864, ((0, 67108863),)),
            ('offset_pack_pointing_onepass', 66304, 512, (0, 1), 'b3', (0, 1), 'b4', (2, 3), 131840,
             67108864, 17, 132096, 67108864, 34, (2, 1), 132352, 67108864, 68, 67108864, ((0, 67108863),),
             'b0+536870912', 'b1+2147483648', 'b2+16', 'b6+536870912'),
            ('release', 'b3', 1073741824),
            ('release', 'b4', 3221225472),
            ('release', 'b5', 16),
            ('release', 'b6', 1610612736),
            ('release', 'b0', 1342177280),
            ('release', 'b1', 5368709120),
            ('release', 'b2', 40),
        ],
        bytes=None,
        plan_dropped=False,
        release_log=[],
    ),
    'otf_temporary_fails': dict(
        result=None,
        log=[
            ('malloc', 1342177280, -2),
            ('malloc', 5368709120, -2),
            ('malloc', 40, -2),
            ('malloc', 1073741824, -2),
            ('malloc_fails', 3221225472, -2),
            ('release', 'b0', 1342177280),
            ('release', 'b1', 5368709120),
            ('release', 'b2', 40),
            ('release', 'b3', 1073741824),
        ],
        bytes=None,
        plan_dropped=False,
        release_log=[],
    ),
    'otf_no_room': dict(
        result=None,
        log=[],
        bytes=None,
        plan_dropped=False,
        release_log=[],
    ),
    'otf_same_identity': dict(
        result={'key': 'b0', 'qu': 'b1', 'cal': 'b2', 'corr': 'b6', 'pair': True, 'blocks': [('b0', 1342177280), ('b1',
            5368709120), ('b2', 40), ('b6', 1610612736)]},
        log=[
            ('malloc', 1342177280, -2),
            ('malloc', 5368709120, -2),
            ('malloc', 40, -2),
            ('malloc', 1073741824, -2),
            ('malloc', 3221225472, -2),
            ('malloc', 16, -2),
            ('malloc', 1610612736, -2),
            ('otf_pixels_healpix', ('pt', 'd0', 'd1'), (0, 1), 'b3', 67108864, ((0, 67108863),), 'b5', 12,
             512),
            ('otf_stokes_weights', ('pt', 'd0', 'd1'), (0, 1), 'b4', 67108864, ((0, 67108863),)),
            ('offset_pack_pointing_onepass', 66304, 512, (0, 1), 'b3', (0, 1), 'b4', (0, 1), 131840,
             67108864, 17, 132096, 67108864, 34, (4, 3), 132352, 67108864, 68, 67108864, ((0, 67108863),),
             'b0', 'b1', 'b2', 'b6'),
            ('otf_pixels_healpix', ('pt', 'd2', 'd3'), (0, 1), 'b3', 67108864, ((0, 67108863),), 'b5', 12,
             512),
            ('otf_stokes_weights', ('pt', 'd2', 'd3'), (0, 1), 'b4', 67108864, ((0, 67108863),)),
            ('offset_pack_pointing_onepass', 66304, 512, (0, 1), 'b3', (0, 1), 'b4', (2, 3), 131840,
             67108864, 17, 132096, 67108864, 34, (2, 1), 132352, 67108864, 68, 67108864, ((0, 67108863),),
             'b0+536870912', 'b1+2147483648', 'b2+16', 'b6+536870912'),
            ('otf_pixels_healpix', ('pt', 'd4'), (0,), 'b3', 67108864, ((0, 67108863),), 'b5', 12, 512),
            ('otf_stokes_weights', ('pt', 'd4'), (0,), 'b4', 67108864, ((0, 67108863),)),
            ('offset_pack_pointing_onepass', 66304, 512, (0,), 'b3', (0,), 'b4', (4,), 131840, 67108864, 17,
             132096, 67108864, 34, (0,), 132352, 67108864, 68, 67108864, ((0, 67108863),), 'b0+1073741824',
             'b1+4294967296', 'b2+32', 'b6+1073741824'),
            ('release', 'b3', 1073741824),
            ('release', 'b4', 3221225472),
            ('release', 'b5', 16),
        ],
        bytes=14,
        again_same_object=True,
        again_result={'key': 'b0', 'qu': 'b1', 'cal': 'b2', 'corr': 'b6', 'pair': True, 'blocks': [('b0', 1342177280), ('b1',
            5368709120), ('b2', 40), ('b6', 1610612736)]},
        again_log=[],
        plan_dropped=True,
        release_log=[
            ('release', 'b0', 1342177280),
            ('release', 'b1', 5368709120),
            ('release', 'b2', 40),
            ('release', 'b6', 1610612736),
        ],
    ),
    'otf_outside_a_solve': dict(
        result=None,
        log=[],
        bytes=None,
        plan_dropped=False,
        release_log=[],
    ),
}


ROUTES = {
    'pair_sums': dict(
        first_half=[
            ('memset', 65792, 0, 86016),
            ('memset', 67072, 0, 96),
            ('offset_accumulate_packed', 25, (0, 3, 6, 9, 12), (2,), 66560, 66816, 65792, 196864, 197120,
             197376, (0.5, 0.5, 0.5, 0.5, 0.5), 8, ((0, 7),), ('pair_corr', 197632), ('pair_words', True)),
            ('otf_offset_accumulate', ('pt', 'd0', 'd1', 'd2'), 25, (0, 3, 6), (2,), 66560, 66816, 66304,
             65792, 512, (0, 1, 2), 131840, 6, (0.5, 0.5, 0.5), 17, 6, ((0, 5),), 132096, 6, 34),
            ('offset_accumulate', 25, (0, 3), (2,), 66560, 66816, 66304, 65792, 512, 3, (0, 1), 131344, (1,
             2), 131600, (0, 1), 131840, 10, (0.5, 0.5), 17, 10, ((0, 9),), 132096, 10, 34),
        ],
        second_half=[
            ('cov_apply_diag', 7, 512, 3, 66048, 65792),
            ('offset_scan_project_packed', 25, (0, 3, 6, 9, 12), (2,), 66560, 67072, 66816, 65792, 196864,
             197120, 197376, (0.5, 0.5, 0.5, 0.5, 0.5), 8, ((0, 7),), ('pair_corr', 197632), ('pair_words',
             True)),
            ('otf_offset_scan_project', ('pt', 'd0', 'd1', 'd2'), 25, (0, 3, 6), (2,), 66560, 67072, 66816,
             66304, 65792, 512, (2, 1, 0), 132352, 6, 68, (0.5, 0.5, 0.5), 6, ((0, 5),)),
            ('offset_scan_project', 25, (0, 3), (2,), 66560, 67072, 66816, 66304, 65792, 512, 3, (0, 1),
             131344, (1, 2), 131600, (1, 0), 132352, 68, (0.5, 0.5), 10, ((0, 9),)),
        ],
        rhs_loop=[
            ('offset_scan_project_signal', 25, (0, 3, 6, 9, 12), (2,), (0, 1, 2, 3, 4), 262144, 67072,
             66816, 66304, 65792, 512, 3, (0, 1, 2, 3, 4), 131328, (1, 2, 3, 4, 5), 131584, (4, 3, 2, 1, 0),
             132352, 68, (0.5, 0.5, 0.5, 0.5, 0.5), 8, ((0, 7),)),
            ('otf_offset_scan_project_signal', ('pt', 'd0', 'd1', 'd2'), 25, (0, 3, 6), (2,), (10, 11, 12),
             262145, 67072, 66816, 66304, 65792, 512, (2, 1, 0), 132352, 6, 68, (0.5, 0.5, 0.5), 6, ((0,
             5),)),
            ('offset_scan_project_signal', 25, (0, 3), (2,), (20, 21), 262146, 67072, 66816, 66304, 65792,
             512, 3, (0, 1), 131344, (1, 2), 131600, (1, 0), 132352, 68, (0.5, 0.5), 10, ((0, 9),)),
        ],
    ),
    'pair_words_only': dict(
        first_half=[
            ('memset', 65792, 0, 86016),
            ('memset', 67072, 0, 96),
            ('offset_accumulate_packed', 25, (0, 3, 6, 9, 12), (2,), 66560, 66816, 65792, 196864, 197120,
             197376, (0.5, 0.5, 0.5, 0.5, 0.5), 8, ((0, 7),), ('pair_corr', 0), ('pair_words', True)),
            ('otf_offset_accumulate', ('pt', 'd0', 'd1', 'd2'), 25, (0, 3, 6), (2,), 66560, 66816, 66304,
             65792, 512, (0, 1, 2), 131840, 6, (0.5, 0.5, 0.5), 17, 6, ((0, 5),), 132096, 6, 34),
            ('offset_accumulate', 25, (0, 3), (2,), 66560, 66816, 66304, 65792, 512, 3, (0, 1), 131344, (1,
             2), 131600, (0, 1), 131840, 10, (0.5, 0.5), 17, 10, ((0, 9),), 132096, 10, 34),
        ],
        second_half=[
            ('cov_apply_diag', 7, 512, 3, 66048, 65792),
            ('offset_scan_project_packed', 25, (0, 3, 6, 9, 12), (2,), 66560, 67072, 66816, 65792, 196864,
             197120, 197376, (0.5, 0.5, 0.5, 0.5, 0.5), 8, ((0, 7),), ('pair_corr', 0), ('pair_words',
             True)),
            ('otf_offset_scan_project', ('pt', 'd0', 'd1', 'd2'), 25, (0, 3, 6), (2,), 66560, 67072, 66816,
             66304, 65792, 512, (2, 1, 0), 132352, 6, 68, (0.5, 0.5, 0.5), 6, ((0, 5),)),
            ('offset_scan_project', 25, (0, 3), (2,), 66560, 67072, 66816, 66304, 65792, 512, 3, (0, 1),
             131344, (1, 2), 131600, (1, 0), 132352, 68, (0.5, 0.5), 10, ((0, 9),)),
        ],
        rhs_loop=[
            ('offset_scan_project_signal', 25, (0, 3, 6, 9, 12), (2,), (0, 1, 2, 3, 4), 262144, 67072,
             66816, 66304, 65792, 512, 3, (0, 1, 2, 3, 4), 131328, (1, 2, 3, 4, 5), 131584, (4, 3, 2, 1, 0),
             132352, 68, (0.5, 0.5, 0.5, 0.5, 0.5), 8, ((0, 7),)),
            ('otf_offset_scan_project_signal', ('pt', 'd0', 'd1', 'd2'), 25, (0, 3, 6), (2,), (10, 11, 12),
             262145, 67072, 66816, 66304, 65792, 512, (2, 1, 0), 132352, 6, 68, (0.5, 0.5, 0.5), 6, ((0,
             5),)),
            ('offset_scan_project_signal', 25, (0, 3), (2,), (20, 21), 262146, 67072, 66816, 66304, 65792,
             512, 3, (0, 1), 131344, (1, 2), 131600, (1, 0), 132352, 68, (0.5, 0.5), 10, ((0, 9),)),
        ],
    ),
    'prior': dict(
        first_half=[
            ('memset', 65792, 0, 86016),
            ('memset', 67072, 0, 96),
            ('add_prior', 'amps_in', 'amps_out'),
            ('offset_accumulate_packed', 25, (0, 3, 6, 9, 12), (2,), 66560, 66816, 65792, 196864, 197120,
             197376, (0.5, 0.5, 0.5, 0.5, 0.5), 8, ((0, 7),), ('pair_corr', 197632), ('pair_words', True)),
            ('otf_offset_accumulate', ('pt', 'd0', 'd1', 'd2'), 25, (0, 3, 6), (2,), 66560, 66816, 66304,
             65792, 512, (0, 1, 2), 131840, 6, (0.5, 0.5, 0.5), 17, 6, ((0, 5),), 132096, 6, 34),
            ('offset_accumulate', 25, (0, 3), (2,), 66560, 66816, 66304, 65792, 512, 3, (0, 1), 131344, (1,
             2), 131600, (0, 1), 131840, 10, (0.5, 0.5), 17, 10, ((0, 9),), 132096, 10, 34),
        ],
        second_half=[
            ('cov_apply_diag', 7, 512, 3, 66048, 65792),
            ('offset_scan_project_packed', 25, (0, 3, 6, 9, 12), (2,), 66560, 67072, 66816, 65792, 196864,
             197120, 197376, (0.5, 0.5, 0.5, 0.5, 0.5), 8, ((0, 7),), ('pair_corr', 197632), ('pair_words',
             True)),
            ('otf_offset_scan_project', ('pt', 'd0', 'd1', 'd2'), 25, (0, 3, 6), (2,), 66560, 67072, 66816,
             66304, 65792, 512, (2, 1, 0), 132352, 6, 68, (0.5, 0.5, 0.5), 6, ((0, 5),)),
            ('offset_scan_project', 25, (0, 3), (2,), 66560, 67072, 66816, 66304, 65792, 512, 3, (0, 1),
             131344, (1, 2), 131600, (1, 0), 132352, 68, (0.5, 0.5), 10, ((0, 9),)),
        ],
        rhs_loop=[
            ('offset_scan_project_signal', 25, (0, 3, 6, 9, 12), (2,), (0, 1, 2, 3, 4), 262144, 67072,
             66816, 66304, 65792, 512, 3, (0, 1, 2, 3, 4), 131328, (1, 2, 3, 4, 5), 131584, (4, 3, 2, 1, 0),
             132352, 68, (0.5, 0.5, 0.5, 0.5, 0.5), 8, ((0, 7),)),
            ('otf_offset_scan_project_signal', ('pt', 'd0', 'd1', 'd2'), 25, (0, 3, 6), (2,), (10, 11, 12),
             262145, 67072, 66816, 66304, 65792, 512, (2, 1, 0), 132352, 6, 68, (0.5, 0.5, 0.5), 6, ((0,
             5),)),
            ('offset_scan_project_signal', 25, (0, 3), (2,), (20, 21), 262146, 67072, 66816, 66304, 65792,
             512, 3, (0, 1), 131344, (1, 2), 131600, (1, 0), 132352, 68, (0.5, 0.5), 10, ((0, 9),)),
        ],
    ),
    'owner_computes': dict(
        first_half=[
            ('memset', 65792, 0, 86016),
            ('memset', 67072, 0, 96),
            ('offset_accumulate_packed', 25, (0, 3, 6, 9, 12), (2,), 66560, 66816, 65792, 196864, 197120,
             197376, (0.5, 0.5, 0.5, 0.5, 0.5), 8, ((0, 7),), ('pair_corr', 197632), ('pair_words', True)),
            ('otf_offset_accumulate', ('pt', 'd0', 'd1', 'd2'), 25, (0, 3, 6), (2,), 66560, 66816, 66304,
             65792, 512, (0, 1, 2), 131840, 6, (0.5, 0.5, 0.5), 17, 6, ((0, 5),), 132096, 6, 34),
            ('offset_accumulate', 25, (0, 3), (2,), 66560, 66816, 66304, 65792, 512, 3, (0, 1), 131344, (1,
             2), 131600, (0, 1), 131840, 10, (0.5, 0.5), 17, 10, ((0, 9),), 132096, 10, 34),
        ],
        second_half=[
            ('comm_map_reduce_apply', 3584, 3, 66048, 65792, ('reduce', True)),
            ('offset_scan_project_packed', 25, (0, 3, 6, 9, 12), (2,), 66560, 67072, 66816, 65792, 196864,
             197120, 197376, (0.5, 0.5, 0.5, 0.5, 0.5), 8, ((0, 7),), ('pair_corr', 197632), ('pair_words',
             True)),
            ('otf_offset_scan_project', ('pt', 'd0', 'd1', 'd2'), 25, (0, 3, 6), (2,), 66560, 67072, 66816,
             66304, 65792, 512, (2, 1, 0), 132352, 6, 68, (0.5, 0.5, 0.5), 6, ((0, 5),)),
            ('offset_scan_project', 25, (0, 3), (2,), 66560, 67072, 66816, 66304, 65792, 512, 3, (0, 1),
             131344, (1, 2), 131600, (1, 0), 132352, 68, (0.5, 0.5), 10, ((0, 9),)),
        ],
        rhs_loop=[
            ('offset_scan_project_signal', 25, (0, 3, 6, 9, 12), (2,), (0, 1, 2, 3, 4), 262144, 67072,
             66816, 66304, 65792, 512, 3, (0, 1, 2, 3, 4), 131328, (1, 2, 3, 4, 5), 131584, (4, 3, 2, 1, 0),
             132352, 68, (0.5, 0.5, 0.5, 0.5, 0.5), 8, ((0, 7),)),
            ('otf_offset_scan_project_signal', ('pt', 'd0', 'd1', 'd2'), 25, (0, 3, 6), (2,), (10, 11, 12),
             262145, 67072, 66816, 66304, 65792, 512, (2, 1, 0), 132352, 6, 68, (0.5, 0.5, 0.5), 6, ((0,
             5),)),
            ('offset_scan_project_signal', 25, (0, 3), (2,), (20, 21), 262146, 67072, 66816, 66304, 65792,
             512, 3, (0, 1), 131344, (1, 2), 131600, (1, 0), 132352, 68, (0.5, 0.5), 10, ((0, 9),)),
        ],
    ),
}


@pytest.mark.parametrize("name", list(case.PACK_SCENARIOS))
def test_pack_scenario(name, install, monkeypatch):
    """Every call, allocation (size, flag -2) and release, in order; what came back; and -- inside ``case.play`` -- that
    after ``release_packed()`` nothing is live, nothing was released twice or with another size than it was taken with."""
    got = case.play(Api(), install, monkeypatch.setenv, **case.PACK_SCENARIOS[name])
    want = PACKS[name]
    assert got["log"] == want["log"]
    assert got == want


def test_pack_scenarios_reach_what_they_are_for():
    """The literals themselves: each scenario took the branch it is named after."""
    names = lambda log: [e[0] for e in log]      # noqa: E731
    for name in ("guard_odd_n_samp", "guard_nnz_1", "guard_no_detectors", "guard_outside_a_solve", "guard_env_off",
                 "guard_trait_off", "otf_outside_a_solve"):
        assert PACKS[name]["result"] is None and PACKS[name]["log"] == [] and PACKS[name]["release_log"] == []
        assert not PACKS[name]["plan_dropped"]
    for name in ("cached_no_room", "otf_no_room"):
        assert PACKS[name]["result"] is None and PACKS[name]["log"] == []
    assert [PACKS[n]["bytes"] for n in ("cached_TTT", "cached_TTF", "cached_TFF", "cached_F")] == [14, 18, 20, None]
    assert "offset_pack_pair_weights" not in names(PACKS["cached_TTF"]["log"])          # (kept as it is: DESIGN.md)
    for name, corr in (("cached_no_pair_sum_block_weights_accepted", "b4"),
                       ("cached_no_pair_sum_block_weights_refused", 0)):
        assert names(PACKS[name]["log"])[3:] == ["malloc_fails", "offset_pack_pointing", "malloc",
                                                 "offset_pack_pair_weights"] + ["release"] * (not corr)
        assert PACKS[name]["result"]["corr"] == corr
    assert names(PACKS["cached_onepass_off"]["log"]) == ["malloc"] * 3 + ["offset_pack_pointing", "malloc",
                                                                           "offset_pack_pair_weights"]
    assert names(PACKS["cached_pair_weights_off"]["log"]) == ["malloc"] * 3 + ["offset_pack_pointing"]
    assert PACKS["cached_second_block_fails"]["log"] == [("malloc", 160, -2), ("malloc_fails", 640, -2),
                                                         ("release", "b0", 160)]
    assert PACKS["cached_second_block_fails"]["result"] is None
    for name in ("cached_same_identity", "otf_same_identity"):
        assert PACKS[name]["again_same_object"] and PACKS[name]["again_log"] == []
    again = names(PACKS["cached_changed_identity"]["again_log"])
    assert again[:4] == ["release"] * 4 and again[4:8] == ["malloc"] * 4
    assert not PACKS["cached_changed_identity"]["again_same_object"]
    # on the fly: row offsets of the batches (b0 = 0, 2, 4), temporaries released after the sweep
    n = case.N_OTF
    sweeps = [e for e in PACKS["otf_TTT"]["log"] if e[0] == "offset_pack_pointing_onepass"]
    assert [e[-4:] for e in sweeps] == [
        tuple(f"b{k}+{off}" if off else f"b{k}" for k, off in ((0, 4 * b0 * n), (1, 16 * b0 * n), (2, 8 * b0),
                                                              (6, 8 * (b0 // 2) * n))) for b0 in (0, 2, 4)]
    assert names(PACKS["otf_TTT"]["log"])[-3:] == ["release"] * 3
    assert [e[1] for e in PACKS["otf_TTT"]["log"][-3:]] == ["b3", "b4", "b5"]
    redo = PACKS["otf_second_batch_without_pair_words"]["log"]
    assert names(redo).count("offset_pack_pointing_onepass") == 2 and names(redo).count("offset_pack_pointing") == 3
    assert all(e[-1] == ("pair_words", False) for e in redo if e[0] == "offset_pack_pointing")
    assert names(redo).count("offset_pack_pairs") == 1 and ("release", "b6", 8 * 3 * n) in redo
    assert names(redo)[-2:] == ["malloc", "offset_pack_pair_weights"]
    bad = PACKS["otf_second_batch_not_ok"]
    assert bad["result"] is None
    assert [e[1] for e in bad["log"] if e[0] == "release"] == ["b3", "b4", "b5", "b6", "b0", "b1", "b2"]
    fails = PACKS["otf_temporary_fails"]
    assert fails["result"] is None and names(fails["log"]) == ["malloc"] * 4 + ["malloc_fails"] + ["release"] * 4
    assert [e[1] for e in fails["log"][-4:]] == ["b0", "b1", "b2", "b3"]


@pytest.mark.parametrize("name", list(case.ROUTE_SCENARIOS))
def test_route_scenario(name, install):
    """The argument tuples of ``accumulate``, ``scan_project`` and ``scan_project_signal``, position by position."""
    got = case.play_routes(Api(), install, **case.ROUTE_SCENARIOS[name])
    assert got == ROUTES[name]


def test_route_and_bytes_per_sample():
    for corr, nbytes in ((True, 14), (False, 18)):
        ctx = Api.context(case.ctx_fields(), case.route_passes(corr))
        assert tuple(ps.route for ps in ctx.passes) == ("packed", "fused-otf", "fused")
        assert tuple(None if ps.pk is None else ps.pk.bytes_per_sample for ps in ctx.passes) == (nbytes, None, None)
    assert PackedPointing().bytes_per_sample == 20


def test_prior_and_owner_computes_in_the_literals():
    names = lambda log: [e[0] for e in log]      # noqa: E731
    assert names(ROUTES["prior"]["first_half"])[:4] == ["memset", "memset", "add_prior", "offset_accumulate_packed"]
    assert "add_prior" not in names(ROUTES["pair_sums"]["first_half"])
    assert names(ROUTES["owner_computes"]["second_half"])[0] == "comm_map_reduce_apply"
    assert "cov_apply_diag" not in names(ROUTES["owner_computes"]["second_half"])
    assert names(ROUTES["pair_sums"]["second_half"])[0] == "cov_apply_diag"


def test_release_is_idempotent_and_covers_a_partial_pack(install):
    fake = case.FakeCapi()
    install(fake)
    pk = PackedPointing()
    pk.key = pk.take(64)
    pk.qu = pk.take(256)
    pk.release()
    pk.release()
    assert fake.take_log() == [("malloc", 64, -2), ("malloc", 256, -2), ("release", "b0", 64), ("release", "b1", 256)]
    assert fake.live == {} and pk.blocks == []


def test_expansion_bound_is_a_named_constant():
    assert packed_pointing.PACK_EXPAND_BYTES == 4 << 30
