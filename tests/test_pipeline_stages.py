"""The stages ``era5_svd._device_pipeline`` is made of, where they can be taken alone on the CPU: the residency
decision (a pure function of byte counts), the vote that makes it one decision for all ranks, and the two fp32
routes of the ingest against each other."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from kernel_double import CpuKernelDouble

GIB = 1 << 30
# a rank's share of X: 1e6 space points x 1000 snapshots, 2 GiB of reserve next to it, 4 ranks
SHAPE = dict(rows=1_000_000, n=1000, rows_all=4_000_000, world_size=4)
RESERVE = 2 * GIB
NEED = 4 * SHAPE["rows"] * SHAPE["n"] + RESERVE


def test_a_slice_that_fits_is_resident():
    from dmd_era5_amd.era5_svd import _stream_bytes_for

    for can_stream in (True, False):
        assert _stream_bytes_for(NEED, NEED, RESERVE, can_stream, **SHAPE) == 0
        assert _stream_bytes_for(NEED, 200 * GIB, RESERVE, can_stream, **SHAPE) == 0


@pytest.mark.parametrize("free,want", [(2 * GIB, 1 << 30), (12 * GIB, 12 * GIB // 3), (200 * GIB, 32 << 30)],
                         ids=["2GiB", "12GiB", "200GiB"])
def test_a_slice_that_does_not_fit_is_streamed_in_pieces_of_a_third_of_the_free_memory(free, want):
    """... clamped to 1 GiB .. 32 GiB."""
    from dmd_era5_amd.era5_svd import _stream_bytes_for

    assert _stream_bytes_for(free + 1, free, RESERVE, True, **SHAPE) == want
    # this rank fits, another one does not: the same path, sized by this rank's free memory
    assert _stream_bytes_for(free, free, RESERVE, True, **SHAPE, others_fit=False) == want


@pytest.mark.parametrize("free", [2 * GIB, 4 * GIB], ids=["2GiB", "4GiB"])
def test_a_slice_that_can_be_neither_resident_nor_streamed_is_refused_with_a_rank_count(free):
    from dmd_era5_amd.era5_svd import _stream_bytes_for

    with pytest.raises(MemoryError, match=r"does not fit.*torch\.distributed\.run.* N >= (\d+)") as ei:
        _stream_bytes_for(NEED, free, RESERVE, False, **SHAPE)
    ranks = int(ei.value.args[0].split("N >= ")[1].split()[0])
    # 16 GB of X over ranks that have max(free - reserve, 1 GiB) each for it, and never fewer than one more than now
    assert ranks == max(-(-4 * SHAPE["rows_all"] * SHAPE["n"] // max(free - RESERVE, GIB)), SHAPE["world_size"] + 1)
    assert ranks >= SHAPE["world_size"] + 1
    assert f"{SHAPE['rows']} x {SHAPE['n']} fp32 = 4.0 GB" in ei.value.args[0]
    # with few enough values the count is the floor: one more rank than there are
    with pytest.raises(MemoryError, match=r"N >= 5 "):
        _stream_bytes_for(NEED, 200 * GIB, RESERVE, False, **dict(SHAPE, rows_all=1000), others_fit=False)


def _vote_worker(rank, world, port, q):
    for p in (os.path.dirname(os.path.abspath(__file__)), os.path.dirname(os.path.dirname(os.path.abspath(__file__)))):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch.distributed as dist

    from dmd_era5_amd import era5_svd
    from dmd_era5_amd import svd as dsvd

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        comm = dsvd.TorchDistComm()
        free = (200 if rank == 0 else 2) * GIB                      # rank 1's share does not fit
        others = era5_svd._all_ranks_fit(NEED <= free, comm, torch.device("cpu"))
        q.put((rank, others, comm.n_collectives,
               era5_svd._stream_bytes_for(NEED, free, RESERVE, True, **dict(SHAPE, world_size=world), others_fit=others)))
    finally:
        dist.destroy_process_group()


def test_one_rank_that_does_not_fit_makes_every_rank_stream():
    """The resident and the streamed run exchange differently, so the ranks must take the same one.  Two gloo ranks,
    rank 1 with too little free memory: both stream, each in pieces sized by its own free memory.  (The wrapper
    around the vote, ``_decide_stream_bytes``, measures a GPU's free memory and returns at once for any other device:
    the vote and the decision are taken here as it calls them.)"""
    from dmd_era5_amd import era5_svd
    from dmd_era5_amd import svd as dsvd

    assert era5_svd._all_ranks_fit(True, dsvd.Comm(), torch.device("cpu")) is True        # one rank: no exchange
    assert era5_svd._all_ranks_fit(False, dsvd.Comm(), torch.device("cpu")) is False
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = [ctx.Process(target=_vote_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = sorted(q.get(timeout=120) for _ in range(2))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert got == [(0, False, 1, 32 << 30), (1, False, 1, 1 << 30)]


@pytest.mark.parametrize("band", [None, (5, 17)], ids=["whole", "band"])
def test_direct_and_host_route_of_the_ingest_give_the_same_blocks(tmp_path, monkeypatch, band):
    """A file-backed fp32 variable with contiguous snapshots and every level is read straight into the pinned
    staging buffers; the same selection of the in-memory array is sliced and copied on the host.  25 snapshots in
    slabs of 7 (whole) or 21 (the band of 12 latitude rows): the last slab is short."""
    from dmd_era5_amd import era5_svd, hdf5_lite, io_netcdf
    from dmd_era5_amd.create_mock_data import create_mock_era5

    if not hdf5_lite.available():
        pytest.fail("libhdf5 not found: a file-backed variable needs the project's HDF5 binding")
    monkeypatch.setenv("DMDX_NETCDF_BACKEND", "hdf5")
    monkeypatch.setattr(era5_svd, "SLAB_BYTES", 7 * 3 * 36 * 72 * 4)
    ds = create_mock_era5("2019-01-01", "2019-01-02", ["temperature"], [1000, 850, 500], seed=5, dtype=np.float32)
    assert ds["temperature"].shape == (25, 3, 36, 72)
    path = str(tmp_path / "slice.nc")
    io_netcdf.to_netcdf(ds, path)
    got = {}
    for route, lazy_bytes in (("direct", 1000), ("host", 1 << 40)):
        monkeypatch.setattr(io_netcdf, "LAZY_BYTES", lazy_bytes)
        da = io_netcdf.open_dataset(path)["temperature"]
        reads = []
        if route == "direct":
            assert da.lazy is not None and da.lazy.dtype == np.float32
            for fn in ("read_slab", "read_box"):
                inner = getattr(da.lazy, fn)
                setattr(da.lazy, fn, lambda a, b, out=None, _f=inner: (reads.append(out is not None), _f(a, b, out))[1])
        else:
            assert da.lazy is None
        st = {"mean": [], "std": []}
        blocks, m_v, nbytes = era5_svd._upload_variable(da, np.arange(3), np.arange(25), torch.device("cpu"),
                                                        CpuKernelDouble(), True, False, st, band)
        got[route] = (blocks, m_v, nbytes, st["mean"], reads)
    (bd, md, nd, mud, reads), (bh, mh, nh, muh, _) = got["direct"], got["host"]
    nlat = 36 if band is None else 12
    assert reads == [True] * (4 if band is None else 2)               # every slab went straight into a staging buffer
    assert md == mh == 3 * nlat * 72 and nd == nh == 4 * 25 * md
    assert len(bd) == len(bh) and sum(int(b.shape[1]) for b in bd) == md
    for x, y in zip(bd + mud, bh + muh):
        assert x.shape == y.shape and torch.equal(x.view(torch.int32), y.view(torch.int32))
