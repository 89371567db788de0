"""HipGraphExecutor._graphed captures with the garbage collector held off (onnx_exec._garbage_collected_first): an automatic collection inside a
stream capture could run the finaliser of a dead engine or pipeline there, whose hipDeviceSynchronize / hipFree a capturing thread must not call.
Checked with a finaliser in plain Python: it has run before the captured walk starts, the collector is off during that walk only, and capture and
replay give the eager result."""
import gc

import pytest
import torch

pytestmark = pytest.mark.gpu


class _Cyclic:
    def __init__(self, log):
        self.me, self.log = self, log

    def __del__(self):
        self.log.append("finalised")


def test_capture_runs_with_the_collector_off():
    from pdf_table_amd.engine import HipEngine
    from pdf_table_amd.onnx_exec import HipGraphExecutor
    ex = object.__new__(HipGraphExecutor)            # _graphed needs the engine's device and the three caches only
    ex.eng, ex._graphs, ex._bad, ex._seen = HipEngine(0), {}, set(), set()
    log = []

    def walk(t):
        log.append(("walk", gc.isenabled()))
        return t * 2.0 + 1.0

    x = torch.arange(12, dtype=torch.float32, device="cuda").reshape(1, 2, 2, 3)
    assert gc.isenabled()
    eager = ex._graphed("k", x, walk).clone()        # first call: eager, remembered
    _Cyclic(log)
    captured = ex._graphed("k", x, walk).clone()     # second call: capture + replay
    replayed = ex._graphed("k", x + 1.0, walk).clone()
    assert log == [("walk", True), "finalised", ("walk", False)]
    assert gc.isenabled() and len(ex._graphs) == 1 and not ex._bad
    assert torch.equal(eager, x * 2.0 + 1.0) and torch.equal(captured, eager) and torch.equal(replayed, (x + 1.0) * 2.0 + 1.0)
    ex.eng.close()
