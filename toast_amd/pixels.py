"""Distributed pixel-domain containers (reference: src/toast/pixels.py:59-241 PixelDistribution,
:436-538 PixelData, :710-780 sync_allreduce) and covariance helpers
(src/toast/covariance.py:20-306).

MI355X-native difference: the map reduction across processes runs **on the device copy**
with one RCCL all-reduce over xGMI (``torch.distributed`` backend "nccl"), instead of
device->host copy, chunked host MPI_Allreduce and host->device copy
(mapmaker_utils.py:885-925 in the reference).  Without a device copy (or with the gloo
backend in CPU tests) the host buffer is reduced."""

import numpy as np

from .accel import (
    AcceleratorObject,
    Resident,
    accel_data_create,
    accel_data_delete,
    accel_data_present,
    accel_data_reset,
    accel_data_update_device,
    accel_data_update_host,
    accel_device_ptr,
    accel_hold,
    make_resident,
    native,
)


class PixelDistribution:
    """Which submaps of the ``n_pix`` pixel domain are held locally."""

    def __init__(self, n_pix=None, n_submap=1000, local_submaps=None, comm=None):
        self._n_pix = int(n_pix)
        self._n_submap = int(n_submap)
        if self._n_submap > self._n_pix:
            raise RuntimeError("Cannot create a PixelDistribution with more submaps than pixels")
        self._n_pix_submap = self._n_pix // self._n_submap
        if self._n_pix % self._n_submap != 0:
            self._n_pix_submap += 1
        self._comm = comm
        if local_submaps is None:
            self._local_submaps = None
            self._glob2loc = None
        else:
            self._local_submaps = np.array(local_submaps, dtype=np.int64)
            if self._local_submaps.size and np.max(self._local_submaps) > self._n_submap - 1:
                raise RuntimeError("local submap indices out of range")
            # pixels.py:216-241
            self._glob2loc = np.full(self._n_submap, -1, dtype=np.int64)
            self._glob2loc[self._local_submaps] = np.arange(self._local_submaps.size, dtype=np.int64)
        self.nest = True

    comm = property(lambda self: self._comm)
    n_pix = property(lambda self: self._n_pix)
    n_submap = property(lambda self: self._n_submap)
    n_pix_submap = property(lambda self: self._n_pix_submap)
    local_submaps = property(lambda self: self._local_submaps)
    global_submap_to_local = property(lambda self: self._glob2loc)

    @property
    def n_local_submap(self):
        return 0 if self._local_submaps is None else int(self._local_submaps.size)

    def __eq__(self, other):
        return (
            isinstance(other, PixelDistribution)
            and self._n_pix == other._n_pix
            and self._n_submap == other._n_submap
            and np.array_equal(self._local_submaps, other._local_submaps)
        )

    def __ne__(self, other):
        return not self.__eq__(other)

    def global_pixel_to_submap(self, gl):
        """pixels.py:193-211: (local submap, pixel within submap); negatives stay negative."""
        gl = np.asarray(gl, dtype=np.int64)
        if gl.size == 0:
            return (np.zeros_like(gl), np.zeros_like(gl))
        if np.max(gl) >= self._n_pix:
            raise RuntimeError("Global pixel indices exceed the maximum for the pixelization")
        bad = gl < 0
        sm = gl // self._n_pix_submap
        pix = gl - sm * self._n_pix_submap
        lsm = np.where(bad, -1, self._glob2loc[np.where(bad, 0, sm)])
        return lsm, np.where(bad, -1, pix)

    def global_pixel_to_local(self, gl):
        """pixels.py:214-236: index into the flat local buffer, local_submap * n_pix_submap + pixel in submap."""
        gl = np.asarray(gl, dtype=np.int64)
        if gl.size == 0:
            return np.zeros_like(gl)
        local_sm, pixels = self.global_pixel_to_submap(gl)
        return pixels + local_sm * self._n_pix_submap

    def clear(self):
        """pixels.py:130-141: drop the global -> local table (the object must not be used afterwards)."""
        self._glob2loc = None

    def __repr__(self):
        return "<PixelDistribution {} pixels, {} submaps, submap size = {}>".format(
            self._n_pix, self._n_submap, self._n_pix_submap)

    def _world(self):
        c = self._comm
        return None if (c is None or c.comm_world is None) else c

    @property
    def all_hit_submaps(self):
        """Submaps local to at least one process (pixels.py:176-185)."""
        if getattr(self, "_all_hit_submaps", None) is None:
            hits = np.zeros(self._n_submap, dtype=np.int64)
            if self._local_submaps is not None:
                hits[self._local_submaps] += 1
            if self._world() is not None:
                self._world().allreduce_array_(hits)
            self._all_hit_submaps = np.flatnonzero(hits != 0)
        return self._all_hit_submaps

    @property
    def submap_owners(self):
        """Owning process of every hit submap, -1 elsewhere (pixels.py:244-297): the hit submaps are dealt out in
        rank order, uniformly (the reference's distribute_uniform: the first `total % size` processes get one more)."""
        if getattr(self, "_submap_owners", None) is not None:
            return self._submap_owners
        owners = np.full(self._n_submap, -1, dtype=np.int32)
        w = self._world()
        if w is None:
            if self._local_submaps is not None and len(self._local_submaps) > 0:
                owners[self._local_submaps] = 0
        else:
            hit = self.all_hit_submaps
            size = w.world_size
            base, extra = divmod(hit.size, size)
            target = [base + (1 if r < extra else 0) for r in range(size)]
            proc = proc_offset = 0
            for sm in hit:
                owners[sm] = proc
                proc_offset += 1
                if proc_offset >= target[proc]:
                    proc += 1
                    proc_offset = 0
        self._submap_owners = owners
        return owners

    @property
    def owned_submaps(self):
        """Submaps owned by this process (pixels.py:299-315)."""
        if getattr(self, "_owned_submaps", None) is None:
            w = self._world()
            rank = 0 if w is None else w.world_rank
            self._owned_submaps = np.flatnonzero(self.submap_owners == rank).astype(np.int32)
        return self._owned_submaps



    @property
    def replicated(self):
        """True when every process holds the same local submaps (the layout of one process per GPU after
        ``unify_local_submaps``): the owner-computes collectives can then run as reduce-scatter / all-gather over
        contiguous pixel shards of the one buffer all ranks share the shape of."""
        if getattr(self, "_replicated", None) is None:
            w = self._world()
            if w is None:
                self._replicated = True
            else:
                mine = np.zeros(self._n_submap, dtype=np.int64)
                if self._local_submaps is not None:
                    mine[self._local_submaps] = 1
                lo, hi = mine.copy(), mine.copy()
                w.allreduce_array_(lo, op="min")
                w.allreduce_array_(hi, op="max")
                self._replicated = bool(np.array_equal(lo, hi))
        return self._replicated

    @property
    def alltoallv_info(self):
        """(send_counts, send_displ, recv_counts, recv_displ, recv_locations) of the submap exchange with the owners, in
        units of submaps (reference pixels.py:317-414).  A process sends each of its local submaps to that submap's
        owner; an owner receives, process by process in rank order, the submaps it owns that the sender holds, each
        in increasing submap order.  ``recv_locations[sm]`` lists the slots of the copies of owned submap ``sm`` in the
        receive buffer.  Local submaps must be sorted (owners then appear in rank order along the local buffer)."""
        if getattr(self, "_alltoallv_info", None) is not None:
            return self._alltoallv_info
        w = self._world()
        local = np.zeros(0, dtype=np.int64) if self._local_submaps is None else self._local_submaps
        if w is None:
            one = np.array([local.size], dtype=np.int32)
            zero = np.zeros(1, dtype=np.int32)
            self._alltoallv_info = (one, zero, one.copy(), zero.copy(),
                                    {int(sm): np.array([k], dtype=np.int32) for k, sm in enumerate(local)})
            return self._alltoallv_info
        if np.any(np.diff(local) <= 0):
            raise RuntimeError("alltoallv needs the local submaps in increasing order")
        size, rank = w.world_size, w.world_rank
        owners = self.submap_owners
        holds = np.zeros(self._n_submap, dtype=np.uint8)
        holds[local] = 1
        holds = w.allgather_array(holds).astype(bool)            # [size, n_submap]
        send_counts = np.bincount(owners[local], minlength=size).astype(np.int32)
        send_displ = (np.cumsum(send_counts) - send_counts).astype(np.int32)
        owned = np.flatnonzero(owners == rank)
        copies = holds[:, owned]                                  # [sender, owned submap]
        recv_counts = copies.sum(axis=1).astype(np.int32)
        recv_displ = (np.cumsum(recv_counts) - recv_counts).astype(np.int32)
        slot = (np.cumsum(copies.ravel()) - 1).reshape(copies.shape)
        recv_locations = {int(sm): slot[copies[:, j], j].astype(np.int32) for j, sm in enumerate(owned)
                          if copies[:, j].any()}
        self._alltoallv_info = (send_counts, send_displ, recv_counts, recv_displ, recv_locations)
        return self._alltoallv_info


def unify_local_submaps(hit_submaps, comm):
    """Union of hit submaps over all processes (one-off MAX all-reduce): every process then
    holds the same ``local_submaps`` so that the per-iteration map reduction is a plain
    all-reduce of one contiguous buffer."""
    hits = np.asarray(hit_submaps).astype(np.int32)
    if comm is not None and comm.comm_world is not None:
        comm.allreduce_array_(hits, op="max")
    return hits.astype(np.uint8)


class PixelData(AcceleratorObject):
    """``[n_local_submap, n_pix_submap, n_value]`` values of a distributed map."""

    def __init__(self, dist, dtype, n_value=1, units=None):
        super().__init__("PixelData")
        self._dist = dist
        self._n_value = int(n_value)
        self._dtype = np.dtype(dtype)
        self.units = units
        self._shape = (dist.n_local_submap, dist.n_pix_submap, self._n_value)
        self._raw = np.zeros(int(np.prod(self._shape)), dtype=self._dtype)
        self._data = self._raw.reshape(self._shape)
        self._pristine = True   # host side still all zero and never handed out (one way: never set back to True)

    distribution = property(lambda self: self._dist)
    n_value = property(lambda self: self._n_value)
    dtype = property(lambda self: self._dtype)

    # Lazy host coherence (like DetectorData.data): Pipelines leave maps resident and device-current (288 GB of HBM);
    # the first HOST access copies the map back and makes the host the current side again.
    def _host(self):
        if self._raw is not None and self._accel_used:
            self.accel_update_host()
        self._pristine = False

    @property
    def raw(self):
        """Flat host buffer (pixels.py:560-563)."""
        self._host()
        return self._raw

    @property
    def data(self):
        """Host view [n_local_submap, n_pix_submap, n_value] (pixels.py:556-558)."""
        self._host()
        return self._data

    @property
    def buffer(self):
        """The flat buffer WITHOUT synchronisation: its address is the accelerator key and its contents may be stale.
        For device-side code paths only."""
        return self._raw

    def arg(self, use_accel):
        """Array to hand to a kernel call: the key view when the kernel runs on the registered device memory, the
        synchronised host contents when the call is host-staged."""
        return self._data if use_accel else self.data

    def host_is_zero(self):
        """True when the host side holds only zeros (without reading it when it was never handed out)."""
        return self._pristine or not np.any(self._raw)

    # array access to the local submaps (pixels.py:613-627)
    def __getitem__(self, key):
        return np.array(self.data[key], dtype=self._dtype, copy=False)

    def __setitem__(self, key, value):
        self.data[key] = value

    def __delitem__(self, key):
        raise NotImplementedError("Cannot delete individual memory elements")

    def __iter__(self):
        return iter(self.data)

    def __len__(self):
        return len(self.data)

    def __repr__(self):
        return "<PixelData {} values per pixel, dtype = {}, units= {}, dist = {}>".format(
            self._n_value, self._dtype.name, self.units, self._dist)

    def clear(self):
        """pixels.py:540-578: release the device copy and the host buffer."""
        if self.accel_exists():
            self.accel_delete()
        self._data = None
        self._raw = None

    def comm_nsubmap(self, bytes):
        """Number of submaps to move per message of about `bytes` bytes (pixels.py:665-683)."""
        dbytes = self._dtype.itemsize
        nsub = int(bytes / (dbytes * self._n_value * self._dist.n_pix_submap))
        if nsub == 0:
            nsub = 1
        allsub = int(self._dist.n_pix / self._dist.n_pix_submap)
        return min(nsub, allsub)

    def _no_device_comm(self):
        if self.accel_in_use():
            raise RuntimeError(f"PixelData {self._accel_name} currently on accelerator cannot do MPI communication")

    def stats(self, comm_bytes=10000000):
        """Sum / mean / rms of every value over all pixels of the hit submaps, on rank zero (None elsewhere); the map
        must already be consistent across processes (pixels.py:972-1093: every submap counted once, contributed by
        the lowest rank holding it; sample variance over all pixels of the hit submaps)."""
        self._no_device_comm()
        dist = self._dist
        w = dist._world()
        if w is None:
            return {
                "sum": [np.sum(self.data[:, :, x]) for x in range(self._n_value)],
                "mean": [np.mean(self.data[:, :, x]) for x in range(self._n_value)],
                "rms": [np.std(self.data[:, :, x]) for x in range(self._n_value)],
            }
        nsub = dist.n_submap
        lowest = np.full(nsub, w.world_size, dtype=np.int64)
        if dist.local_submaps is not None:
            lowest[dist.local_submaps] = w.world_rank
        w.allreduce_array_(lowest, op="min")
        mine = np.flatnonzero(lowest == w.world_rank)
        loc = dist.global_submap_to_local[mine]
        # the reference counts n_pix_submap pixels for EVERY submap index (hit or not: unhit ones contribute zeros)
        count = float(nsub) * dist.n_pix_submap
        part = np.array([np.sum(self.data[loc, :, v], dtype=np.float64) for v in range(self._n_value)])
        w.allreduce_array_(part)
        mean = part / count
        n_unhit = nsub - np.count_nonzero(lowest < w.world_size)
        var = np.array([np.sum((self.data[loc, :, v].astype(np.float64) - mean[v]) ** 2)
                        for v in range(self._n_value)])
        w.allreduce_array_(var)
        var += n_unhit * dist.n_pix_submap * mean**2
        if w.world_rank != 0:
            return None
        return {
            "sum": [float(x) for x in part],
            "mean": [float(x) for x in mean],
            "rms": [float(np.sqrt(x / (count - 1))) for x in var],
        }

    def broadcast_map(self, fdata, comm_bytes=10000000):
        """Distribute a full map held by process zero: `fdata` = one array of n_pix values per map value (or a single
        array when n_value == 1), significant on process zero only; every process keeps its local submaps
        (pixels.py:1095-1184: chunks of submaps are broadcast; pixels past n_pix in the last submap are zero)."""
        self._no_device_comm()
        dist = self._dist
        w = dist._world()
        rank = 0 if w is None else w.world_rank
        nps = dist.n_pix_submap
        if rank == 0 and self._n_value == 1 and not isinstance(fdata, (tuple, list)):
            fdata = (fdata,)
        comm_submap = self.comm_nsubmap(comm_bytes)
        buf = np.zeros((comm_submap, nps, self._n_value), dtype=self._dtype)
        for sm0 in range(0, dist.n_submap, comm_submap):
            nsm = min(comm_submap, dist.n_submap - sm0)
            buf[:] = 0
            if rank == 0:
                p0 = sm0 * nps
                p1 = min((sm0 + nsm) * nps, dist.n_pix)
                flat = buf.reshape(-1, self._n_value)
                for col in range(self._n_value):
                    flat[: p1 - p0, col] = np.asarray(fdata[col])[p0:p1]
            if w is not None:
                w.bcast_array_(buf, root=0)
            for sm in range(sm0, sm0 + nsm):
                loc = dist.global_submap_to_local[sm]
                if loc >= 0:
                    self.data[loc, :, :] = buf[sm - sm0, :, :]

    def update_units(self, units):
        self.units = units

    def reset(self):
        if self.accel_in_use():
            self.accel_reset()   # the device copy is the current one; the host side is refreshed on access
            return
        if not self._pristine:
            # the buffer has been handed out (.raw / .data / a view): a caller may still hold it and write after this
            # reset, so the "known zero" shortcut is gone for good -- host_is_zero() looks at the contents from now on
            self._raw[:] = 0
        if self.accel_exists():
            self.accel_reset()

    def duplicate(self):
        """Copy of the current side: device-to-device when the map is in use there (the host side of the copy is
        refreshed on access), host-to-host otherwise."""
        if self.accel_in_use():
            return self.duplicate_on_device()
        dup = PixelData(self._dist, self._dtype, n_value=self._n_value, units=self.units)
        if not self._pristine:
            dup._raw[:] = self._raw
            dup._pristine = False
        return dup

    def duplicate_on_device(self):
        """Copy whose DEVICE side is filled by a device-to-device copy (the source must be in use on the
        device); the host side of the copy stays zero until ``accel_update_host``.  Spares the D2H + H2D
        round trip of ``duplicate`` for intermediates that are consumed on the device."""
        from . import capi

        if not self.accel_in_use():
            raise RuntimeError("duplicate_on_device: the data is not in use on the device")
        dup = PixelData(self._dist, self._dtype, n_value=self._n_value, units=self.units)
        with accel_hold(self):      # a failed allocation must not evict the source of the copy
            dup.accel_create(self._accel_name + "_copy")
        capi.dev.copy(accel_device_ptr(dup._raw), accel_device_ptr(self._raw), self._raw.nbytes)
        dup.accel_used(True)
        return dup

    def _device_collectives(self, comm):
        """True when this map's collectives go through the library's RCCL communicator on the kernels' stream.

        The answer depends only on things that are the same on every rank -- the communicator, the distribution, the
        dtype -- never on where THIS rank's copy of the map happens to live: a rank that has evicted its map
        (Data.accel_evict under memory pressure, uneven detector shards) must enter the same collective on the same
        communicator as the others, or the job hangs.  A host-resident copy is uploaded for the collective and
        brought back afterwards (``_device_side``)."""
        from . import capi

        return bool(comm.device_comm() and self._dist.replicated and self._dtype in capi.dev.COMM_DTYPES
                    and self._raw is not None and self._raw.size > 0)

    def _union_on_device(self, comm):
        """Ranks that hold DIFFERENT local submaps (the reference's general case, pixels.py:792-940): the default exchange
        -- every submap becomes the sum of its copies -- runs on the device through the UNION of all ranks' submaps.
        Like _device_collectives, the answer is the same on every rank (``replicated`` is a collective property)."""
        from . import capi

        return bool(comm.device_comm() and self._dtype in capi.dev.COMM_DTYPES and not self._dist.replicated)

    def _union_exchange(self):
        """sync_alltoallv() with the default local_func for a distribution whose ranks hold different submaps: the local
        submaps are moved into their places in a zeroed scratch map over the union of all ranks' submaps
        (toast_hip_block_move_dev), that map is summed over the ranks like a replicated one (owner computes /
        all-reduce, on the kernels' stream), and the local submaps are read back.  A submap nobody else holds comes
        back as it was; a rank without local submaps takes part with zeros."""
        from . import capi

        D = capi.dev
        dist = self._dist
        union = dist.all_hit_submaps
        if union.size == 0:
            return
        local = np.asarray(dist.local_submaps if dist.local_submaps is not None else [], dtype=np.int64)
        pos = np.searchsorted(union, local).astype(np.int64)
        here = np.arange(local.size, dtype=np.int64)
        block = self._n_submap_value * self._raw.itemsize
        nbytes = int(union.size) * block
        scratch = capi.device_malloc(nbytes, -4 if nbytes < (1 << 30) else -1)
        try:
            D.memset(scratch, 0, nbytes)

            def reduce():
                if self._dtype == np.float64:
                    D.comm_map_reduce_apply(int(union.size) * self._dist.n_pix_submap, self._n_value, 0, scratch,
                                            reduce=True)
                else:
                    D.comm_allreduce(scratch, int(union.size) * self._n_submap_value, self._dtype, "sum")

            if local.size > 0:
                with self._device_side():
                    D.block_move(scratch, accel_device_ptr(self._raw), block, pos, here)
                    reduce()
                    D.block_move(accel_device_ptr(self._raw), scratch, block, here, pos)
            else:
                reduce()
        finally:
            capi.device_free(scratch)      # (waits for the stream)
        self._pristine = False

    def _device_side(self):
        """Context manager: inside, the device copy is the current one; a copy that lived on the host is uploaded on
        entry, downloaded on exit, and a device buffer created for the purpose is released again."""
        import contextlib

        @contextlib.contextmanager
        def ctx():
            mine = Resident(self, self._accel_name)
            try:
                yield
            finally:
                if mine.uploaded:
                    self.accel_update_host()
                    mine.drop_if_created()

        return ctx()

    def sync_allreduce(self, comm=None, comm_bytes=10000000):
        """Sum the map over all processes; every process ends with the total (reference pixels.py:710-780; all
        processes must hold the same local submaps).  Device-resident data: one in-place RCCL all-reduce enqueued on
        the kernels' stream -- no host synchronisation before or after, the next kernel simply follows in stream
        order.  ``comm_bytes`` (the reference's message size on the host) has no meaning here."""
        del comm_bytes
        comm = self._dist.comm if comm is None else comm
        if comm is None or comm.comm_world is None:
            return
        if self._device_collectives(comm):
            from . import capi

            with self._device_side():
                capi.dev.comm_allreduce(accel_device_ptr(self._raw), self._raw.size, self._dtype, "sum")
            return
        restore = False
        if self.accel_in_use():
            self.accel_update_host()
            restore = True
        self._pristine = False
        comm.allreduce_array_(self._raw)
        if restore:
            self.accel_update_device()

    # ---- owner-computes exchange (reference pixels.py:780-967)
    @property
    def _n_submap_value(self):
        return self._dist.n_pix_submap * self._n_value

    @staticmethod
    def local_reduction(n_submap_value, receive_locations, receive, reduce_buf):
        """Default ``local_func``: every owned submap becomes the sum of its copies (pixels.py:780-789)."""
        for locs in receive_locations.values():
            reduce_buf[:] = 0
            for lc in locs:
                reduce_buf += receive[lc:lc + n_submap_value]
            for lc in locs:
                receive[lc:lc + n_submap_value] = reduce_buf

    def setup_alltoallv(self):
        """Counts, displacements and the persistent receive / reduce buffers of the exchange (pixels.py:791-876)."""
        if getattr(self, "_send_counts", None) is not None:
            return
        send_counts, send_displ, recv_counts, recv_displ, recv_locations = self._dist.alltoallv_info
        scale = self._n_submap_value
        self._send_counts = scale * np.asarray(send_counts, dtype=np.int64)
        self._send_displ = scale * np.asarray(send_displ, dtype=np.int64)
        self._recv_counts = scale * np.asarray(recv_counts, dtype=np.int64)
        self._recv_displ = scale * np.asarray(recv_displ, dtype=np.int64)
        self._recv_locations = {sm: scale * np.asarray(locs, dtype=np.int64) for sm, locs in recv_locations.items()}
        self.reduce_buf = np.zeros(scale, dtype=self._dtype)
        if self._dist._world() is None:
            self.receive = self.raw          # serial: owned submaps are the local ones, in place
        else:
            self.receive = np.zeros(int(self._recv_displ[-1] + self._recv_counts[-1]), dtype=self._dtype)

    def forward_alltoallv(self):
        """Send every local submap to its owner (pixels.py:878-909).  Host data."""
        if self.accel_in_use():
            self.accel_update_host()
        self.setup_alltoallv()
        w = self._dist._world()
        if w is None:
            return
        w.alltoallv_array(self.raw, self._send_counts, self._send_displ, self.receive, self._recv_counts,
                          self._recv_displ)

    def reverse_alltoallv(self):
        """Send the owners' copies back to every holder (pixels.py:911-939)."""
        w = self._dist._world()
        if w is None:
            return
        if getattr(self, "_send_counts", None) is None:
            raise RuntimeError("Cannot do reverse alltoallv before buffers have been setup")
        w.alltoallv_array(self.receive, self._recv_counts, self._recv_displ, self.raw, self._send_counts,
                          self._send_displ)

    def sync_alltoallv(self, local_func=None, comm=None):
        """Owner-computes exchange (reference pixels.py:942-967): every submap goes to its owner, ``local_func(
        n_submap_value, receive_locations, receive, reduce_buf)`` works on the owned submaps there (default: sum of the
        copies), the results go back to every holder.

        Device-resident data held with the same local submaps on every rank runs as RCCL reduce-scatter -> per-pixel
        kernel on the owned pixel shard -> all-gather on the kernels' stream, when ``local_func`` is the default or
        one of the covariance functors of this module (``create_local_apply / _invert / _multiply``: they carry the
        device form of their operation).  Any other ``local_func`` runs on the host with the reference's buffers."""
        if comm is not None and comm is not self._dist.comm:
            raise RuntimeError("sync_alltoallv works on the communicator of the pixel distribution")
        w = self._dist._world()
        if w is None and local_func is None:
            return      # one process: every submap is its own and only copy
        device_form = local_func is None or hasattr(local_func, "on_device")
        if w is not None and local_func is None and self._union_on_device(w):
            self._union_exchange()
            return
        if w is not None and device_form and self._device_collectives(w):
            with self._device_side():
                if local_func is None:
                    from . import capi

                    if self._dtype == np.float64:
                        capi.dev.comm_map_reduce_apply(self._raw.size // self._n_value, self._n_value, 0,
                                                       accel_device_ptr(self._raw), reduce=True)
                    else:   # integer / single precision maps: the plain all-reduce gives the same sums
                        capi.dev.comm_allreduce(accel_device_ptr(self._raw), self._raw.size, self._dtype, "sum")
                else:
                    local_func.on_device(self)
            return
        restore = self.accel_in_use()
        self.forward_alltoallv()
        self._pristine = False
        if local_func is None:
            local_func = self.local_reduction
        local_func(self._n_submap_value, self._recv_locations, self.receive, self.reduce_buf)
        self.reverse_alltoallv()
        if restore:
            self.accel_update_device()

    # accelerator protocol
    def _accel_exists(self):
        return self._raw is not None and self._raw.size > 0 and accel_data_present(self._raw, self._accel_name)

    def _accel_create(self, zero_out=False):
        # a map is what the A^T kernels scatter into with atomics: the arena keeps it away from the zone of the arrays
        # that feed the scatter (KIND_SCATTER; a covariance or hit map is only written once -- same place, no harm)
        accel_data_create(self._raw, self._accel_name, zero_out=zero_out, owner=self, kind=2)

    def _accel_update_device(self):
        accel_data_update_device(self._raw, self._accel_name)

    def _accel_update_host(self):
        accel_data_update_host(self._raw, self._accel_name)
        self._pristine = False

    def _accel_delete(self):
        accel_data_delete(self._raw, self._accel_name)

    def _accel_reset(self):
        accel_data_reset(self._raw, self._accel_name)


# ----------------------------------------------------------------------------- covariance
def _mapnnz(npp):
    return int(((np.sqrt(8 * npp.n_value) - 1) / 2) + 0.5)


def _owner_computes_on_device(pd):
    w = pd.distribution._world()
    return w is not None and pd._device_collectives(w)


class _LocalFunc:
    """A ``local_func`` of ``PixelData.sync_alltoallv`` (signature ``(n_submap_value, receive_locations, receive,
    reduce_buf)``, reference covariance.py:34-75, 134-177, 224-259) that also knows its device form ``on_device(pd)``:
    the per-pixel kernel on this rank's pixel shard followed by the all-gather."""


class create_local_apply(_LocalFunc):
    """m <- cov . m on the owned submaps; the copies of a submap are taken to be equal (the map was reduced before),
    the first one is multiplied and written to every location (covariance.py:224-259).  ``cov`` must have gone
    through ``forward_alltoallv`` for the host form."""

    def __init__(self, n_pix_submap, mapnnz, cov):
        self.n_pix_submap, self.mapnnz, self.cov = n_pix_submap, mapnnz, cov

    def __call__(self, n_submap_value, receive_locations, receive, reduce_buf):
        cov = self.cov
        n_cov = self.n_pix_submap * cov.n_value
        for sm, locs in receive_locations.items():
            c0 = cov._recv_locations[sm][0]
            reduce_buf[:] = receive[locs[0]:locs[0] + n_submap_value]
            cov.reduce_buf[:] = cov.receive[c0:c0 + n_cov]
            native().cov_apply_diag(1, self.n_pix_submap, self.mapnnz, cov.reduce_buf, reduce_buf, False)
            for lc in locs:
                receive[lc:lc + n_submap_value] = reduce_buf

    def on_device(self, m, reduce=False):
        from . import capi

        with accel_hold(m):
            make_resident(self.cov, "covariance")
        capi.dev.comm_map_reduce_apply(m.buffer.size // m.n_value, self.mapnnz, accel_device_ptr(self.cov.buffer),
                                       accel_device_ptr(m.buffer), reduce=reduce)


class create_local_invert(_LocalFunc):
    """Eigendecomposition / inverse of the owned submaps' blocks with the condition-number threshold
    (covariance.py:34-75): the first copy is processed and written to every location; ``rcond`` (optional PixelData,
    ``setup_alltoallv`` done) receives the inverse condition numbers."""

    def __init__(self, n_pix_submap, mapnnz, threshold, rcond, invert=False):
        self.n_pix_submap, self.mapnnz, self.threshold, self.rcond, self.invert = (n_pix_submap, mapnnz, threshold,
                                                                                   rcond, invert)

    def __call__(self, n_submap_value, receive_locations, receive, reduce_buf):
        rcond = self.rcond
        for sm, locs in receive_locations.items():
            reduce_buf[:] = receive[locs[0]:locs[0] + n_submap_value]
            if rcond is None:
                rdata = np.zeros(self.n_pix_submap)
            else:
                rcond.reduce_buf[:] = 0.0
                rdata = rcond.reduce_buf
            native().cov_eigendecompose_diag(1, self.n_pix_submap, self.mapnnz, reduce_buf, rdata, float(self.threshold),
                                             bool(self.invert), False)
            for lc in locs:
                receive[lc:lc + n_submap_value] = reduce_buf
            if rcond is not None:
                for lc in rcond._recv_locations[sm]:
                    rcond.receive[lc:lc + self.n_pix_submap] = rcond.reduce_buf

    def on_device(self, npp):
        from . import capi

        rcond = self.rcond
        d_rc = 0
        if rcond is not None:
            with accel_hold(npp):
                if not rcond.accel_exists():
                    rcond.accel_create("rcond", zero_out=True)
            d_rc = accel_device_ptr(rcond.buffer)
        capi.dev.comm_cov_invert(npp.buffer.size // npp.n_value, self.mapnnz, accel_device_ptr(npp.buffer), d_rc,
                                 float(self.threshold), invert=self.invert)
        if rcond is not None:
            rcond.accel_used(True)


class create_local_multiply(_LocalFunc):
    """npp1 <- npp1 . npp2 on the owned submaps (covariance.py:134-177); ``other`` must have gone through
    ``forward_alltoallv`` for the host form."""

    def __init__(self, n_pix_submap, mapnnz, other):
        self.n_pix_submap, self.mapnnz, self.other = n_pix_submap, mapnnz, other

    def __call__(self, n_submap_value, receive_locations, receive, reduce_buf):
        other = self.other
        for sm, locs in receive_locations.items():
            o0 = other._recv_locations[sm][0]
            reduce_buf[:] = receive[locs[0]:locs[0] + n_submap_value]
            other.reduce_buf[:] = other.receive[o0:o0 + n_submap_value]
            native().cov_mult_diag(1, self.n_pix_submap, self.mapnnz, reduce_buf, other.reduce_buf, False)
            for lc in locs:
                receive[lc:lc + n_submap_value] = reduce_buf

    def on_device(self, npp1):
        from . import capi

        with accel_hold(npp1):
            make_resident(self.other, "covariance2")
        capi.dev.comm_cov_mult(npp1.buffer.size // npp1.n_value, self.mapnnz, accel_device_ptr(npp1.buffer),
                               accel_device_ptr(self.other.buffer))


def covariance_apply(npp, m, use_alltoallv=False):
    """In-place ``m <- npp . m`` per pixel (reference: src/toast/covariance.py:262-306).  Runs where the map lives: on
    the device copies when the map is resident there.  ``use_alltoallv``: every process multiplies only the submaps
    it owns and the results are exchanged (on the device: its pixel shard, then an all-gather)."""
    mapnnz = _mapnnz(npp)
    if npp.distribution != m.distribution:
        raise RuntimeError("covariance matrix and map must have same pixel distribution")
    if m.n_value != mapnnz:
        raise RuntimeError("covariance matrix and map have incompatible NNZ values")
    if use_alltoallv and m.distribution._world() is not None:
        lapply = create_local_apply(npp.distribution.n_pix_submap, mapnnz, npp)
        if _owner_computes_on_device(m):
            with m._device_side():
                lapply.on_device(m)
        else:
            npp.forward_alltoallv()
            m.sync_alltoallv(local_func=lapply)
        return
    on_dev = m.accel_in_use()
    if on_dev:
        with accel_hold(m):
            make_resident(npp, "covariance")
    elif npp.accel_in_use():
        npp.accel_update_host()
    native().cov_apply_diag(npp.distribution.n_local_submap, npp.distribution.n_pix_submap, mapnnz,
                            npp.buffer if on_dev else npp.raw, m.buffer if on_dev else m.raw, on_dev)


def map_reduce_apply(npp, m, sync_type="alltoallv"):
    """``m <- npp . (sum over processes of m)``: the finalisation of a binned map and the middle of every PCG
    iteration.  With device-resident data and ``sync_type="alltoallv"`` one owner-computes pass -- reduce-scatter,
    ``cov_apply_diag`` on the owned pixel shard, all-gather -- instead of an all-reduce followed by every process
    multiplying the whole map; otherwise ``sync_allreduce`` / ``sync_alltoallv`` followed by ``covariance_apply``."""
    if sync_type == "alltoallv" and _owner_computes_on_device(m):
        with m._device_side():
            create_local_apply(npp.distribution.n_pix_submap, _mapnnz(npp), npp).on_device(m, reduce=True)
        return
    if sync_type == "alltoallv":
        m.sync_alltoallv()
    else:
        m.sync_allreduce()
    covariance_apply(npp, m, use_alltoallv=(sync_type == "alltoallv"))


def covariance_multiply(npp1, npp2, use_alltoallv=False):
    """In-place per-pixel product of two block-diagonal covariances, ``npp1 <- npp1 npp2`` (reference:
    src/toast/covariance.py:179-221 -> cov_mult_diag).  Runs where ``npp1`` lives."""
    mapnnz = _mapnnz(npp1)
    if npp1.distribution != npp2.distribution:
        raise RuntimeError("covariance matrices must have same pixel distribution")
    if npp1.n_value != npp2.n_value:
        raise RuntimeError("covariance matrices must have same n_values")
    if use_alltoallv and npp1.distribution._world() is not None:
        lmult = create_local_multiply(npp1.distribution.n_pix_submap, mapnnz, npp2)
        if _owner_computes_on_device(npp1):
            with npp1._device_side():
                lmult.on_device(npp1)
        else:
            npp2.forward_alltoallv()
            npp1.sync_alltoallv(local_func=lmult)
    else:
        on_dev = npp1.accel_in_use()
        if on_dev:
            with accel_hold(npp1):
                make_resident(npp2, "covariance2")
        elif npp2.accel_in_use():
            npp2.accel_update_host()
        native().cov_mult_diag(npp1.distribution.n_local_submap, npp1.distribution.n_pix_submap, mapnnz,
                               npp1.buffer if on_dev else npp1.raw, npp2.buffer if on_dev else npp2.raw, on_dev)
    if npp1.units is not None and npp2.units is not None:
        try:
            npp1.update_units(npp1.units * npp2.units)
        except TypeError:
            pass


def covariance_invert(npp, threshold, rcond=None, use_alltoallv=False):
    """In-place inverse of the per-pixel blocks with an rcond threshold
    (reference: src/toast/covariance.py:78-131 -> cov_eigendecompose_diag).  Runs where the matrix
    lives: a device-resident covariance is inverted there and stays there (its condition-number map
    too); host data is staged through the GPU by the host-level entry point.  ``use_alltoallv``: every process
    inverts only the submaps it owns (on the device: its pixel shard) and the results are exchanged."""
    mapnnz = _mapnnz(npp)
    if npp.n_value <= 0:
        raise RuntimeError(f"NNZ = {npp.n_value}. It is an error to invert a pixel matrix with non-positive dimensions.")
    if rcond is not None:
        if rcond.distribution != npp.distribution:
            raise RuntimeError("covariance matrix and condition number map must have same pixel distribution")
        if rcond.n_value != 1:
            raise RuntimeError("condition number map should have n_value = 1")
    dist = npp.distribution
    if use_alltoallv and dist._world() is not None:
        linvert = create_local_invert(dist.n_pix_submap, mapnnz, threshold, rcond, invert=True)
        if _owner_computes_on_device(npp):
            with npp._device_side():
                linvert.on_device(npp)
            if rcond is not None and not npp.accel_in_use() and rcond.accel_in_use():
                rcond.accel_update_host()      # (the matrix was only on the device for the collective: so is its rcond)
            return
        if rcond is not None:
            if rcond.accel_in_use():
                rcond.accel_update_host()
            rcond.setup_alltoallv()
        npp.sync_alltoallv(local_func=linvert)
        if rcond is not None:
            rcond._pristine = False
            rcond.reverse_alltoallv()
        return
    if npp.accel_in_use():
        from . import capi

        cond = PixelData(dist, np.float64, n_value=1) if rcond is None else rcond
        with accel_hold(npp):
            if not cond.accel_exists():
                cond.accel_create("rcond", zero_out=True)
        capi.dev.cov_eigendecompose_diag(dist.n_local_submap, dist.n_pix_submap, mapnnz, accel_device_ptr(npp.buffer),
                                         accel_device_ptr(cond.buffer), float(threshold), True)
        cond.accel_used(True)
        if rcond is None:
            native().accel_synchronize()
            cond.accel_delete()
        return
    cond = np.zeros(dist.n_local_submap * dist.n_pix_submap) if rcond is None else rcond.raw
    native().cov_eigendecompose_diag(dist.n_local_submap, dist.n_pix_submap, mapnnz, npp.raw, cond, float(threshold),
                                     True, False)


def covariance_rcond(npp, use_alltoallv=False):
    """Condition-number map of a covariance (reference: covariance.py:190-259)."""
    mapnnz = int(((np.sqrt(8 * npp.n_value) - 1) / 2) + 0.5)
    rcond = PixelData(npp.distribution, np.float64, n_value=1)
    if npp.accel_in_use():
        npp.accel_update_host()
    work = npp.raw.copy()
    native().cov_eigendecompose_diag(npp.distribution.n_local_submap, npp.distribution.n_pix_submap, mapnnz, work,
                                     rcond.raw, 0.0, False, False)
    return rcond
