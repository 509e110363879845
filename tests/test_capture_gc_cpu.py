"""decode.no_gc: the cyclic collector is off inside the block and back in its earlier state behind it (also when the block raises)."""
import gc

import pytest

from valor_amd import decode


def test_no_gc_switches_the_collector_off_and_restores_it():
    assert gc.isenabled()
    with decode.no_gc():
        assert not gc.isenabled()
        with decode.no_gc():                       # nested (a decode capture inside nothing else today, but the state is a stack)
            assert not gc.isenabled()
        assert not gc.isenabled()
    assert gc.isenabled()
    with pytest.raises(KeyError):
        with decode.no_gc():
            raise KeyError("x")
    assert gc.isenabled()
    gc.disable()                                   # a driver that manages the collector itself (TrainEngine(manage_gc=True)): stays off
    try:
        with decode.no_gc():
            assert not gc.isenabled()
        assert not gc.isenabled()
    finally:
        gc.enable()
