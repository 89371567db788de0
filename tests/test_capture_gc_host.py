"""onnx_exec._garbage_collected_first, the guard around HipGraphExecutor's stream capture (no GPU): cyclic garbage is finalised before the guarded
region begins, the collector is off inside it whatever is allocated there, and its earlier state comes back afterwards -- also after an exception."""
import gc

import pytest

from pdf_table_amd import onnx_exec as X


class _Cyclic:
    def __init__(self, log):
        self.me, self.log = self, log

    def __del__(self):
        self.log.append("finalised")


def test_collects_first_and_holds_the_collector_off():
    log = []
    assert gc.isenabled()
    _Cyclic(log)
    with X._garbage_collected_first():
        log.append("inside")
        assert not gc.isenabled()
        _Cyclic(log)
        junk = [[] for _ in range(100000)]           # far beyond the generation-0 threshold: no automatic collection all the same
        del junk
        assert log == ["finalised", "inside"]
    assert gc.isenabled()
    gc.collect()
    assert log == ["finalised", "inside", "finalised"]


def test_restores_the_state_it_found():
    gc.disable()
    try:
        with X._garbage_collected_first():
            assert not gc.isenabled()
        assert not gc.isenabled()
    finally:
        gc.enable()
    with pytest.raises(RuntimeError):
        with X._garbage_collected_first():
            raise RuntimeError("capture failed")
    assert gc.isenabled()
