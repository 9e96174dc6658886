"""GPU tests of the multi-program render kernel (authjx_render_batch_multi_device,
authorino_amd/csrc/ajx_render.hip ajx_render_values_multi): a batch whose requests render
different programs, or none, against one-program calls (authjx_render_batch, pinned to the
Python mirror by tests/test_gpu_render.py) over each program's requests. The per-request
body's CPU checks are tests/test_render_multi_host.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = ("runs", "alternating", "none")


@pytest.fixture(scope="module")
def setup():
    """The context, the three programs (tests/_rendermulti.py) compiled for the device, 513
    fuzz documents and a cache of each batch's values (the oracle's, by n and interleaving)."""
    import _rendermulti as M
    import _rendertest as T
    from authorino_amd import runtime

    ctx = runtime.Context(0)
    progs = M.programs()
    dev = [ctx.compile_render(o, s) for o, s, _ in progs]
    return ctx, progs, dev, T.fuzz_docs(513, seed=23), {}


def _one(ctx, dev):
    import _rendertest as T

    def one(i, docs, values, text, out_text):
        arena, offs, lens = T.pack(docs)
        return ctx.render_host_arena(dev[i], arena, offs, lens, values, text, out_text=out_text)

    return one


def _multi(ctx, dev, por, docs, values, text, out_stride, records_stride, stream=None, guard_rows=1):
    """authjx_render_batch_multi_device into guard-filled device buffers with `guard_rows`
    more rows than requests: (records, out_text) as numpy, status masked where written."""
    import torch

    import _rendermulti as M
    import _rendertest as T

    d = torch.device("cuda", 0)
    arena, offs, lens = T.pack(docs)
    n = len(docs)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(d)  # noqa: E731
    A, Of, Ln = up(arena), up(offs.view(np.int64)), up(lens.view(np.int32))
    P = up(por.view(np.int32)) if por is not None else None
    V, X = up(values.view(np.int32)), up(text)
    out = torch.full((n + guard_rows, out_stride), M.GUARD, dtype=torch.uint8, device=d)
    rec = torch.full((n + guard_rows, max(records_stride, 1), 3), M.GUARD32 - (1 << 32), dtype=torch.int32, device=d)
    torch.cuda.synchronize()
    ctx.render_multi_device(dev, P, A, Of, Ln, V, out, rec, text=X, stream=stream)
    return rec, out


def _fetch(rec, out):
    import _rendermulti as M

    r = rec.cpu().numpy().view(np.uint32).copy()
    M.mask_status(r)
    return r, out.cpu().numpy()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 513])
def test_interleaved_programs_equal_one_program_calls(setup, n):
    """n requests (a single lane; a wave with one idle lane; a wave boundary; the 256-thread
    workgroup boundary of the LDS level stack; two workgroups and one lane) in runs by
    program, strictly alternating and all without a program, at out_stride 16 and 4096:
    records and whole output slots equal the one-program call's over each program's
    requests; requests without a program, the records past a program's own outputs and the
    row after the batch keep their guard bytes."""
    import torch

    import _rendermulti as M

    ctx, progs, dev, docs, cache = setup
    docs = docs[:n]
    for shape in SHAPES:
        por = M.interleaving(n, shape)
        if (n, shape) not in cache:
            cache[(n, shape)] = M.batch_values(progs, por, docs)
        values, text = cache[(n, shape)]
        for out_stride in (16, 4096):
            want_rec, want_out = M.expected(progs, por, docs, values, text, out_stride, _one(ctx, dev))
            rec, out = _multi(ctx, dev, por, docs, values, text, out_stride, 18)
            torch.cuda.synchronize()
            rec, out = _fetch(rec, out)
            assert np.array_equal(rec[:n], want_rec), (shape, out_stride)
            assert np.array_equal(out[:n], want_out), (shape, out_stride)
            assert (out[n] == M.GUARD).all() and (rec[n] == M.GUARD32).all()
            idle = por == M.NONE
            assert (out[:n][idle] == M.GUARD).all() and (rec[:n][idle] == M.GUARD32).all()
            if shape == "alternating" and n >= 63 and out_stride == 4096:
                # (not a comparison of empty things, and the programs are told apart)
                assert (rec[:n][por == 1][:, :18, 2] == 0).all() and (rec[:n][por == 1][:, 17, 1] >= 18).all()
                assert (rec[:n][por == 0][:, :4, 2] == 0).all() and (rec[:n][por == 0][:, 4:] == M.GUARD32).all()


def test_program_lists_change_on_one_stream(setup):
    """Three calls queued back to back on one side stream with the program list in another
    order each time (the stream's pointer table has two slots), then one more with the
    first list: each gives its own list's result."""
    import torch

    import _rendermulti as M

    ctx, progs, dev, docs, _ = setup
    n = 130
    docs = docs[:n]
    stream = torch.cuda.Stream(device=torch.device("cuda", 0))
    runs = []
    for order in ([0, 1, 2], [1, 2, 0], [2, 0, 1], [0, 1, 2]):
        pl, dl = [progs[i] for i in order], [dev[i] for i in order]
        por = M.interleaving(n, "alternating")
        values, text = M.batch_values(pl, por, docs)
        want = M.expected(pl, por, docs, values, text, 512, _one(ctx, dl))
        with torch.cuda.stream(stream):
            runs.append((want, _multi(ctx, dl, por, docs, values, text, 512, 18, stream=stream.cuda_stream)))
    stream.synchronize()
    ctx.release_stream(stream.cuda_stream)
    for k, ((want_rec, want_out), (rec, out)) in enumerate(runs):
        rec, out = _fetch(rec, out)
        assert np.array_equal(rec[:n], want_rec), k
        assert np.array_equal(out[:n], want_out), k


def test_one_program_without_indices_and_einval_table(setup):
    """d_prog_of_req NULL with one program renders it for every request. AUTHJX_EINVAL:
    values_stride or records_stride below a program's need, a NULL program, several
    programs without indices, no programs, out_stride 0 or no multiple of 16, an output
    buffer that is not 16-byte aligned, a NULL buffer; nothing is written by a refused call."""
    import torch

    import _rendermulti as M
    from authorino_amd import runtime

    ctx, progs, dev, docs, _ = setup
    n = 40
    docs = docs[:n]
    por = np.ones(n, dtype=np.uint32)
    values, text = M.batch_values(progs, por, docs)
    want_rec, want_out = M.expected(progs, por, docs, values, text, 256, _one(ctx, dev))
    rec, out = _multi(ctx, [dev[1]], None, docs, values, text, 256, 18)
    torch.cuda.synchronize()
    rec, out = _fetch(rec, out)
    assert np.array_equal(rec[:n], want_rec) and np.array_equal(out[:n], want_out)

    def refused(devs, por_, values_, out_stride, records_stride):
        with pytest.raises(runtime.AuthjxError, match="EINVAL"):
            _multi(ctx, devs, por_, docs, values_, text, out_stride, records_stride)

    refused(dev, None, values, 256, 18)                    # three programs, no indices
    refused([], por, values, 256, 18)                      # no programs
    refused(dev, por, values, 24, 18)                      # out_stride no multiple of 16
    refused(dev, por, values, 256, 17)                     # below the 18 outputs of program 1
    refused(dev, por, values[:, :7].copy(), 256, 18)       # below the 8 slots of program 0
    refused([dev[0], None, dev[2]], por, values, 256, 18)  # a NULL program
    d = torch.device("cuda", 0)
    import _rendertest as T

    arena, offs, lens = T.pack(docs)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(d)  # noqa: E731
    A, Of, Ln, P = up(arena), up(offs.view(np.int64)), up(lens.view(np.int32)), up(por.view(np.int32))
    V, X = up(values.view(np.int32)), up(text)
    slots = torch.full((n * 256 + 16,), M.GUARD, dtype=torch.uint8, device=d)
    rec = torch.full((n, 18, 3), -1, dtype=torch.int32, device=d)
    ok = slots[:n * 256].view(n, 256)
    with pytest.raises(runtime.AuthjxError, match="EINVAL"):  # out_stride 0
        ctx.render_multi_device(dev, P, A, Of, Ln, V, ok[:, :0], rec, text=X)
    with pytest.raises(runtime.AuthjxError, match="EINVAL"):  # not 16-byte aligned
        ctx.render_multi_device(dev, P, A, Of, Ln, V, slots[8:8 + n * 256].view(n, 256), rec, text=X)
    L = runtime.load_library()
    parr = (runtime.C.c_void_p * 3)(*[p._h.value for p in dev])
    rc = L.authjx_render_batch_multi_device(ctx._h, parr, 3, P.data_ptr(), A.data_ptr(), Of.data_ptr(), Ln.data_ptr(),
                                            n, V.data_ptr(), 8, X.data_ptr(), X.shape[1], None, 256, rec.data_ptr(),
                                            18, None)
    assert rc == -1  # a NULL output buffer
    rc = L.authjx_render_batch_multi_device(None, parr, 3, P.data_ptr(), A.data_ptr(), Of.data_ptr(), Ln.data_ptr(),
                                            n, V.data_ptr(), 8, X.data_ptr(), X.shape[1], ok.data_ptr(), 256,
                                            rec.data_ptr(), 18, None)
    assert rc == -1  # no context
    torch.cuda.synchronize()
    assert bool((slots == M.GUARD).all()) and bool((rec == -1).all())
