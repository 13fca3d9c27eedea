"""Scenarios for the solver's packed pointing cache and launch context on the host: a fake ``capi`` (device calls that
log and answer from a script, an allocator that hands out fake addresses and checks every release) and the inputs of
every scenario.  A scenario drives the code under test through an *api* object, so that the same scenario can be played
against another implementation of the same steps (tests/test_packed_pointing_host.py says how its literals were made).

Fields of a pass / a context are spelled as keyword dictionaries; the api turns them into its own types."""

import numpy as np

BASE, STRIDE = 1 << 44, 1 << 40       # fake block k lives at BASE + k * STRIDE (no scenario's block is that long)
TOTAL = 256 << 30
DETS = ["d0", "d1", "d2", "d3", "d4"]


def sym(x):
    """Log form of an argument: "b<k>+<offset>" for an address in fake block k, tuples for arrays."""
    if isinstance(x, np.ndarray):
        return tuple(sym(v) for v in x.tolist())
    if isinstance(x, (list, tuple)):
        return tuple(sym(v) for v in x)
    if isinstance(x, (int, np.integer)) and not isinstance(x, bool) and x >= BASE:
        k, off = divmod(int(x) - BASE, STRIDE)
        return f"b{k}" + (f"+{off}" if off else "")
    if isinstance(x, np.generic):
        return x.item()
    return x


class FakeCapi:
    """``dev``, ``device_malloc``, ``device_release`` and ``accel_mem_info`` of ``toast_amd.capi`` without a device.
    ``answers``: call name -> list of results handed out in turn (the last one repeats)."""

    def __init__(self, answers=None, fail_malloc=(), mem=(200 << 30, TOTAL)):
        self.log, self.live, self.n_malloc = [], {}, 0
        self.answers = {k: list(v) for k, v in (answers or {}).items()}
        self.fail_malloc, self.mem = set(fail_malloc), mem
        self.dev = self

    def install(self):
        """Attributes to put on the capi module (the caller restores them)."""
        return dict(dev=self, device_malloc=self.device_malloc, device_release=self.device_release,
                    accel_mem_info=self.accel_mem_info)

    def device_malloc(self, nbytes, flags=-1):
        k, self.n_malloc = self.n_malloc, self.n_malloc + 1
        if k in self.fail_malloc:
            self.log.append(("malloc_fails", nbytes, flags))
            raise RuntimeError("toast_hip: out of device memory")
        self.log.append(("malloc", nbytes, flags))
        self.live[BASE + k * STRIDE] = nbytes
        return BASE + k * STRIDE

    def device_release(self, ptr, nbytes):
        assert self.live.pop(ptr, None) == nbytes, f"release of {sym(ptr)}, {nbytes} B: not live with that size"
        self.log.append(("release", sym(ptr), nbytes))

    def accel_mem_info(self):
        return self.mem

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)

        def call(*args, **kwargs):
            self.log.append((name,) + sym(args) + tuple(sorted(kwargs.items())))
            turn = self.answers.get(name)
            if not turn:
                return None
            return turn.pop(0) if len(turn) > 1 else turn[0]

        return call

    def take_log(self):
        log, self.log = self.log, []
        return log


def ctx_fields(**over):
    f = dict(on_the_fly=False, nnz=3, nps=512, n_local=7, zmap="zmap", amps_in="amps_in", amps_out="amps_out",
             zmap_ptr=0x10100, zmap_bytes=86016, cov_ptr=0x10200, g2l_ptr=0x10300, in_ptr=0x10400, in_flags_ptr=0x10500,
             out_ptr=0x10600, out_bytes=96, det_flag_mask=17, shared_flag_mask=34, tmpl_flag_mask=68, prior=None,
             owner_computes=False)
    f.update(over)
    return f


def pass_fields(n_det=5, n_samp=8, otf=False, iob=0, **over):
    dets = DETS[:n_det]
    f = dict(iob=iob, dets=dets, step=25, ao=np.arange(n_det, dtype=np.int64) * 3, nav=np.array([2], dtype=np.int64),
             n_samp=n_samp, ivl=np.array([[0, n_samp - 1]], dtype=np.int64), detw=np.full(n_det, 0.5),
             f_idx=np.arange(n_det, dtype=np.int32), f_ptr=0x20300, f_ns=n_samp, s_ptr=0x20400, s_n=n_samp,
             pf_idx=np.arange(n_det, dtype=np.int32)[::-1].copy(), pf_ptr=0x20500, pf_n=n_samp)
    if otf:
        f["pt"] = ("pt",) + tuple(dets)
    else:
        f.update(pi=np.arange(n_det, dtype=np.int32), pp=0x20100, wi=np.arange(n_det, dtype=np.int32) + 1, wp=0x20200)
    f.update(over)
    return f


N_OTF = 2 ** 26          # 5 detectors of this length: the on-the-fly fill works in batches of 2, 2 and 1
OTF_SOURCE = dict(nside=64, nest=True, n_submap=12)


def descriptor(dets):
    return ("pt",) + tuple(dets)


def summary(pk):
    """What a pack request returned, in log form.  ``pk``: None or (key, qu, cal, corr, pair, blocks)."""
    if pk is None:
        return None
    key, qu, cal, corr, pair, blocks = pk
    return dict(key=sym(key), qu=sym(qu), cal=sym(cal), corr=sym(corr), pair=bool(pair),
                blocks=[(sym(p), n) for p, n in blocks])


def play(api, install, setenv, kind, answers=None, fail_malloc=(), mem=(200 << 30, TOTAL), env=None, in_solve=True,
         packed_pointing=True, ctx=None, ps=None, again=None):
    """One pack request (``kind``: "cached" or "otf") on a fresh operator, optionally a second one (``again``: "same" or
    a dictionary of pass fields that differ), then ``release_packed()``.  Returns everything a test compares."""
    fake = FakeCapi(answers, fail_malloc, mem)
    install(fake)
    for k, v in (env or {}).items():
        setenv(k, v)
    otf = kind == "otf"
    c = ctx_fields(on_the_fly=otf, **(ctx or {}))
    p = pass_fields(otf=otf, **dict(dict(n_samp=N_OTF) if otf else {}, **(ps or {})))
    op = api.operator(packed_pointing)
    request = api.pack_otf if otf else api.pack_cached
    first = request(op, c, p, in_solve)
    out = dict(result=summary(api.fields(first)), log=fake.take_log(), bytes=api.bytes_per_sample(first))
    if again is not None:
        p2 = p if again == "same" else dict(p, **again)
        second = request(op, c, p2, in_solve)
        out.update(again_same_object=second is first, again_result=summary(api.fields(second)),
                   again_log=fake.take_log())
    out["plan_dropped"] = api.release(op)
    out["release_log"] = fake.take_log()
    api.release(op)                                    # a second release does nothing
    assert fake.take_log() == [] and fake.live == {}, fake.live
    return out


GOOD = dict(offset_pack_pointing=[(True, True)], offset_pack_pairs=[True], offset_pack_pair_weights=[True])


def onepass(*results):
    return dict(GOOD, offset_pack_pointing_onepass=list(results))


T, F = True, False
# name -> keyword arguments of ``play``
PACK_SCENARIOS = {
    # cached pointing, 5 detectors x 8 samples
    "cached_TTT": dict(kind="cached", answers=onepass((T, T, T))),
    "cached_TTF": dict(kind="cached", answers=onepass((T, T, F))),
    "cached_TFF": dict(kind="cached", answers=onepass((T, F, F))),
    "cached_F": dict(kind="cached", answers=onepass((F, F, F))),
    "cached_no_pair_sum_block_weights_accepted": dict(kind="cached", answers=GOOD, fail_malloc=[3]),
    "cached_no_pair_sum_block_weights_refused": dict(kind="cached", answers=dict(GOOD, offset_pack_pair_weights=[False]),
                                                     fail_malloc=[3]),
    "cached_onepass_off": dict(kind="cached", answers=GOOD, env={"TOAST_HIP_PACK_ONEPASS": "0"}),
    "cached_pair_weights_off": dict(kind="cached", answers=GOOD, env={"TOAST_HIP_PACKED_PAIR_WEIGHTS": "0"}),
    "cached_second_block_fails": dict(kind="cached", answers=GOOD, fail_malloc=[1]),
    # (the three blocks of 5 x 8 take 800 B: one byte short of leaving a fifth of the device free, and exactly enough)
    "cached_no_room": dict(kind="cached", answers=GOOD, mem=(TOTAL // 5 + 799, TOTAL)),
    "cached_just_room": dict(kind="cached", answers=onepass((T, T, T)), mem=(TOTAL // 5 + 800, TOTAL)),
    "guard_odd_n_samp": dict(kind="cached", answers=GOOD, ps=dict(n_samp=7)),
    "guard_nnz_1": dict(kind="cached", answers=GOOD, ctx=dict(nnz=1)),
    "guard_no_detectors": dict(kind="cached", answers=GOOD, ps=dict(n_det=0)),
    "guard_outside_a_solve": dict(kind="cached", answers=GOOD, in_solve=False),
    "guard_env_off": dict(kind="cached", answers=GOOD, env={"TOAST_HIP_PACKED_POINTING": "0"}),
    "guard_trait_off": dict(kind="cached", answers=GOOD, packed_pointing=False),
    "cached_same_identity": dict(kind="cached", answers=onepass((T, T, T)), again="same"),
    "cached_changed_identity": dict(kind="cached", answers=onepass((T, T, T)), again=dict(pp=0x20108)),
    # pointing on the fly, 5 detectors x 2**26 samples: batches of 2, 2 and 1 detectors
    "otf_TTT": dict(kind="otf", answers=onepass((T, T, T))),
    "otf_second_batch_without_pair_words": dict(kind="otf", answers=onepass((T, T, T), (T, F, F))),
    "otf_second_batch_not_ok": dict(kind="otf", answers=onepass((T, T, T), (F, F, F))),
    "otf_temporary_fails": dict(kind="otf", answers=GOOD, fail_malloc=[4]),
    "otf_no_room": dict(kind="otf", answers=GOOD, mem=(TOTAL // 5 + 1000, TOTAL)),
    "otf_same_identity": dict(kind="otf", answers=onepass((T, T, T)), again="same"),
    "otf_outside_a_solve": dict(kind="otf", answers=GOOD, in_solve=False),
}


# -- routes: one context, three passes (packed, pointing on the fly, cached arrays) ----------------------------------
def route_passes(corr):
    """Pass fields of the three observations; the packed one carries its pack as (key, qu, cal, corr, pair, blocks)."""
    packed = pass_fields(iob=0, pk=(0x30100, 0x30200, 0x30300, 0x30400 if corr else 0, True, []))
    otf = pass_fields(iob=1, n_det=3, n_samp=6, otf=True)
    arrays = pass_fields(iob=2, n_det=2, n_samp=10, pp=0x20110, wp=0x20210)
    return [packed, otf, arrays]


def signal_rows(p):
    """(row indices, device pointer) of the right-hand side's timestreams in observation ``p["iob"]``"""
    return np.arange(len(p["dets"]), dtype=np.int32) + 10 * p["iob"], 0x40000 + p["iob"]


class Prior:
    def __init__(self, fake):
        self.fake = fake

    def add_prior(self, amps_in, amps_out):
        self.fake.log.append(("add_prior", amps_in, amps_out))


def play_routes(api, install, corr=True, prior=False, owner_computes=False):
    """Both halves of the left-hand side and the right-hand side's launch loop over the three passes."""
    fake = FakeCapi()
    install(fake)
    c = ctx_fields(owner_computes=owner_computes, prior=Prior(fake) if prior else None)
    passes = route_passes(corr)
    out = {}
    for name in ("first_half", "second_half", "rhs_loop"):
        getattr(api, name)(c, passes)
        out[name] = fake.take_log()
    return out


ROUTE_SCENARIOS = {
    "pair_sums": dict(corr=True),
    "pair_words_only": dict(corr=False),
    "prior": dict(corr=True, prior=True),
    "owner_computes": dict(corr=True, owner_computes=True),
}
