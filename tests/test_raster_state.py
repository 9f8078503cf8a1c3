"""raster.RasterState, the state of one rasterizer call, on CPU tensors: which counter column each total reads, what verify() raises
and when, that it never builds the tile lists, and the read-only state["name"] form."""
import pytest
import torch

from siu3r_amd import raster

V, T = 2, 12
#                      Gv  D   E  flags
STATS = torch.tensor([[5, 40, 17, 0],
                      [7, 90, 23, 0]], dtype=torch.int64)


def _state(cap_e=64, lists=None):
    st = raster.RasterState(V=V, G=9, W=64, H=48, T=T, stats_dev=STATS.clone(), cap_e=cap_e, rec=torch.zeros(V, 9, 12),
                            tiles_touched_all=torch.arange(V * 9, dtype=torch.int32).reshape(V, 9), defer=True)
    if lists is not None:
        cap_d, totals = lists
        tstart = torch.zeros((V, T + 2), dtype=torch.int32)
        tstart[:, T + 1] = torch.tensor(totals, dtype=torch.int32)
        st._tl = (tstart, torch.zeros((V, cap_d), dtype=torch.int32), cap_d)
    return st


@pytest.fixture
def no_library(monkeypatch):
    """any call into the native library (building the tile lists is one) fails the test"""
    def lib():
        raise AssertionError("the state reached for the native library")
    monkeypatch.setattr(raster._lib, "lib", lib)


def test_totals_and_derived_values_read_their_columns(no_library):
    st = _state()
    assert st.totals(0) == [5, 7] and st.totals(1) == [40, 90] and st.totals(2) == [17, 23]
    assert (st.Gv, st.D, st.E) == (5, 40, 17) == (st["Gv"], st["D"], st["E"])  # view 0
    assert torch.equal(st.stats(), STATS) and st.stats() is st.stats()  # one host copy
    assert torch.equal(st.tiles_touched, st.tiles_touched_all[0])


def test_verify_raises_on_entry_overflow_with_the_message(no_library):
    _state(cap_e=23).verify()
    with pytest.raises(raster.RasterOverflow) as exc:
        _state(cap_e=22).verify()
    assert str(exc.value) == "rasterizer coarse-bin entries overflowed: E = 23 > entry_capacity 22 (pass entry_capacity >= 23)"
    assert exc.value.call_id is None


def test_verify_does_not_build_the_lists(no_library):
    st = _state()
    st.verify()  # (no_library: an attempt to build them would have raised)
    assert st._tl is None
    with pytest.raises(AssertionError, match="native library"):  # the lazy properties are what builds them
        st.tile_start_all


def test_verify_checks_the_pair_capacity_of_built_lists(no_library):
    _state(lists=(90, [40, 90])).verify()
    st = _state(lists=(89, [40, 90]))
    with pytest.raises(raster.RasterOverflow) as exc:
        st.verify()
    assert str(exc.value) == "rasterizer tile-pair lists overflowed: D = 90 > pair_capacity 89 (pass pair_capacity >= 90)"
    assert st.cap_d == 89 and st.ids_all.shape == (V, 89) and st.ids.shape == (89,) and st.tile_start.shape == (T + 2,)
    assert st["tile_start_all"] is st.tile_start_all and st["cap_d"] == 89


def test_item_form_is_read_only(no_library):
    st = _state()
    assert st["rec"] is st.rec and st["cap_e"] == 64 and st["feat_ws"] is None
    for name in ("nope", "stats", "verify", "_tl", "_lists"):  # only the public fields and properties are keys
        with pytest.raises(KeyError, match=name):
            st[name]
    with pytest.raises(TypeError):
        st["rec"] = torch.zeros(1)
    with pytest.raises(TypeError):
        st["nope"] = 1
    with pytest.raises(AttributeError):  # every field is declared in the class
        st.nope = 1
    with pytest.raises(AssertionError, match="nope"):
        raster.RasterState(nope=1)
