"""GPU tests of the render kernels (authorino_amd/csrc/ajx_render.hip) over generated values:
tests/render_gen.py's numbers, strings, keys and containers, the cases and checks of
tests/_rendervalues.py that tests/test_render_values_host.py runs on the host build. Render
inputs are the oracle's values (and text slots) fed to authjx_render_batch, so the render
kernel is judged by itself; every expected byte is the Python mirror's, never another run of
the code under test."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CORPUS_SEED, CORPUS_DOCS = 3101, 513


@pytest.fixture(scope="module")
def ctx():
    from authorino_amd import runtime

    return runtime.Context(0)


@pytest.fixture(scope="module")
def corpus():
    """513 generated documents with the oracle's values and the mirror's bytes, once."""
    import _rendervalues as V

    return V.corpus(CORPUS_SEED, CORPUS_DOCS)


@pytest.mark.parametrize("n", [1, 64, 65, 257, 513])
def test_corpus_prefixes(ctx, corpus, n):
    """A lone lane, a wave, a wave plus one, a workgroup plus one, two workgroups plus one:
    every output OK and byte-equal to the mirror, packed back to back, nothing written past a
    request's end, the slot after the batch untouched."""
    import _rendervalues as V

    c = V.prefix(corpus, n)
    rec, out = V.device_render(ctx)(c.outputs, c.n_slots, c.docs, c.vals, c.text, c.stride)
    assert V.check_exact(c, rec, out) == n * 32


def test_device_select_against_oracle(ctx, corpus):
    """authjx_select_text_batch of the same documents (whitespace around every token, depth 8
    below two more levels, escaped keys, 7 KiB): the oracle's (start, len, type) for every
    slot, none unresolved."""
    import _rendertest as T
    import render_gen as G

    rs = ctx.compile([(p, 1, "") for p in G.PATHS], [], -1)
    assert all(s == 0 for s in rs.status)
    arena, offs, lens = T.pack(corpus.docs)
    vals, _ = ctx.select_text_host_arena([rs], arena, offs, lens)
    assert not ((vals[:, :, 2] & 0xFF) == 255).any()
    assert np.array_equal(vals[:, :, :2], corpus.vals[:, :, :2])
    assert np.array_equal(vals[:, :, 2] & 0xFF, corpus.vals[:, :, 2] & 0xFF)


def test_depth_profile(ctx):
    """257 requests whose consecutive lanes hold 1, 6, 3, 8, 5, 2, 7, 4 levels of distinct
    members under SPRINT and MARSHAL: a level stack that leaked between lanes or levels
    would print another lane's member."""
    import _rendervalues as V

    assert V.check_depth_profile(V.device_render(ctx)) == 2 * 257


def test_long_strings(ctx):
    """LIT + each op over strings of up to about 3,000 bytes; out_stride from the mirror's
    longest request."""
    import _rendervalues as V

    assert V.check_long_strings(V.device_render(ctx)) == 4 * 130


def test_fill_levels(ctx):
    """129 corpus documents at out_stride 16 and 64: OK exactly when the mirror's bytes fit
    the room left, else UNRENDERED and the outputs after it still right; an Inf under MARSHAL
    may be either (counted)."""
    import _rendervalues as V

    counts = V.check_fill_levels(V.device_render(ctx), seeds=(CORPUS_SEED,), n=129, strides=(16, 64))
    for stride, (tot, unfit, inf) in counts.items():
        print("out_stride %d: %d outputs, %d did not fit, %d Inf under MARSHAL given as UNRENDERED"
              % (stride, tot, unfit, inf))
        assert 0 < unfit < tot


def test_counts_and_utf8_table(ctx):
    import _rendervalues as V

    assert V.check_counts(V.device_render(ctx)) == 4 * len(V.COUNTS)
    V.check_utf8_table(V.device_render(ctx))


def test_built_text(ctx):
    """One seed of the modifier-chain and "#." list corpus, rendered from the text slot."""
    import _rendervalues as V

    tot, from_text, not_utf8, unsupported = V.check_built(V.device_render(ctx), V.BUILT_SEEDS[:1])
    print("built text: %d outputs, %d from the text slot, %d declined as not UTF-8, %d of type 255"
          % (tot, from_text, not_utf8, unsupported))
    assert from_text > tot // 2 and not_utf8 > 0 and unsupported > 0


def test_multi_program_kernel_against_the_mirror(ctx, corpus):
    """authjx_render_batch_multi_device: the op list split three ways as three programs,
    alternating per request with every fourth request without a program, 257 documents.
    Each program's requests equal the mirror directly; requests without a program, the
    records past a program's own outputs and the row after the batch keep their guard bytes."""
    import torch

    import _rendermulti as M
    import _rendervalues as V
    import render_gen as G
    from test_gpu_render_multi import _fetch, _multi

    n = 257
    c = V.prefix(corpus, n)
    cuts = [0, 11, 22, len(G.OUTPUTS)]
    parts = [G.OUTPUTS[a:b] for a, b in zip(cuts, cuts[1:])]
    dev = [ctx.compile_render(o, G.N_SLOTS) for o in parts]
    por = M.interleaving(n, "alternating")
    rs = max(len(o) for o in parts)
    rec, out = _multi(ctx, dev, por, c.docs, c.vals, c.text, c.stride, rs)
    torch.cuda.synchronize()
    rec, out = _fetch(rec, out)
    for i, (a, b) in enumerate(zip(cuts, cuts[1:])):
        idx = np.flatnonzero(por == i)
        assert len(idx) >= 64
        sub = V.Case(parts[i], G.N_SLOTS, [c.docs[j] for j in idx], c.vals[idx], None,
                     [c.want[j][a:b] for j in idx], c.stride)
        assert (rec[idx][:, b - a:] == M.GUARD32).all()
        V.check_exact(sub, rec[idx][:, :b - a], np.concatenate([out[idx], out[n:]]))
    idle = por == M.NONE
    assert idle.sum() >= 64 and (out[:n][idle] == M.GUARD).all() and (rec[:n][idle] == M.GUARD32).all()
    assert (out[n] == M.GUARD).all() and (rec[n] == M.GUARD32).all()
