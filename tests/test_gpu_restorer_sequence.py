"""-m gpu: the order in which the video restorer calls its own entry points, window by window, with the second option set of
test_gpu_restorer_options.py and ``pipeline=False``: one thread, so the order of the calls is the order on the streams.  Every
caller reaches ``shiftnet_amd.lib.check`` through the module, with the entry point's name as its second argument: a recorder in its place sees every
call, still judges the return code, and keeps the names of the restorer's own entry points (the engines' are not its business).  The lists below are
those the restorer gave before its features moved into restore_parts.py; they are compared with ==."""
import pytest

import test_gpu_restorer_options as O
from shiftnet_amd import lib, restore
from shiftnet_amd.io_edges import yuv_fmt

pytestmark = pytest.mark.gpu

OWN = ("sn_yuv_", "sn_ingest_yuv", "sn_egress_yuv", "sn_noise_map_level", "sn_tile_accumulate")

STAGE = ["sn_yuv_noise_hist_rect", "sn_yuv_block_motion", "sn_yuv_noise_hist_pairs_mv", "sn_yuv_noise_hist_bands", "sn_yuv_noise_hist_pairs_bands_mv",
         "sn_ingest_yuv_rect", "sn_ingest_yuv_rect"]
# the input in the format written (the whole frames, then the rectangle as the cropped stream converts it), the blend, the report
WRITE = ["sn_ingest_yuv", "sn_egress_yuv", "sn_ingest_yuv_rect", "sn_egress_yuv_rect", "sn_egress_yuv_mix", "sn_yuv_diff_stats"]
PAIRS = ["sn_yuv_block_motion", "sn_yuv_diff_stats_mv"]                # of the frames written: a window of one frame has none


def window(tiles, pairs=True, auto=False):
    return (["sn_yuv_rowcol_sums"] if auto else []) + STAGE + ["sn_noise_map_level"] + ["sn_tile_accumulate"] * tiles + WRITE + (PAIRS if pairs else [])


@pytest.fixture
def calls(monkeypatch):
    seen, check = [], lib.check

    def recorder(rc, what):
        if what.startswith(OWN):
            seen.append(what)
        return check(rc, what)

    monkeypatch.setattr(lib, "check", recorder)
    return seen


def by_window(vr, pay, h, w, written, calls):
    """The calls of every window: the serial driver hands a window's frames out before it stages the next."""
    it, out = vr.restore(iter(pay), yuv_fmt(*O.FMT), h, w), []
    for n in written:
        del calls[:]
        for _ in range(n):
            next(it)
        out.append(list(calls))
    del calls[:]
    assert list(it) == [] and calls == []
    return out


def tiles_of(got, per_window):
    """The ``sn_tile_accumulate`` calls of a window: one per tile, and as many again where the range guard tripped and the tiles ran once more."""
    n = got.count("sn_tile_accumulate")
    assert n in (per_window, 2 * per_window)
    return n


@pytest.fixture(scope="module")
def net():
    return restore.load_net("denoise_small", "synthetic", "bf16")


def test_listed_picture_first_and_second_window(net, calls):
    pay, h, w, picture, windows, rect, tiles, per_window = O.CASES["listed_picture"]()
    vr = restore.VideoRestorer(net, O.ONE_LEN, pipeline=False, picture=picture, **dict(O.MORE, **tiles))
    got = by_window(vr, pay, h, w, [4, 1, 4, 2], calls)
    assert [len(t) for t in vr.stats["window_tiles"]] == [per_window] * 4
    assert got[0] == window(tiles_of(got[0], per_window))                # 4 frames written, 8 fed
    assert got[1] == window(tiles_of(got[1], per_window), pairs=False)   # 1 written
    assert got[2] == window(tiles_of(got[2], per_window)) and got[3] == window(tiles_of(got[3], per_window))


def test_auto_picture_starts_every_window_with_the_sums(net, calls):
    pay, h, w, picture, windows, rect, tiles, per_window = O.CASES["auto_picture"]()
    vr = restore.VideoRestorer(net, O.ONE_LEN, pipeline=False, picture=picture, **dict(O.MORE, **tiles))
    got = by_window(vr, pay, h, w, [4, 1, 2], calls)
    assert [g[0] for g in got] == ["sn_yuv_rowcol_sums"] * 3
    for g, pairs in zip(got, (True, False, True)):
        assert g == window(tiles_of(g, per_window), pairs=pairs, auto=True)
