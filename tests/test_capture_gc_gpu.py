"""A dead reference cycle that still owns device resources (an earlier model with its decoding sessions: hipGraphs, private pools) is
freed whenever Python's cyclic collector happens to run. Inside a graph capture those frees are illegal and end the process, and
torch.cuda.graph does not collect before it begins: the decoding step's capture keeps the collector off for its duration."""
import gc

import pytest
import torch

pytestmark = pytest.mark.gpu


def test_collector_is_off_inside_a_decode_step_capture(dev, monkeypatch):
    from valor_amd import decode, synth
    from valor_amd.model.valor import VALOR
    monkeypatch.setenv("VALOR_DECODE_GRAPH", "1")
    spec = synth.tiny_spec()
    m = VALOR({"dropout": 0.0, "max_generation_len": 6}, spec=spec, dtype=torch.float32, device=dev)
    m.load_state_dict(synth.make_state_dict(spec, seed=5, w_std=0.05), strict=True)
    seen = []
    body = decode.DecodeSession._body

    def probe(self, cur):
        seen.append((torch.cuda.is_current_stream_capturing(), gc.isenabled()))
        return body(self, cur)
    monkeypatch.setattr(decode.DecodeSession, "_body", probe)
    batch = synth.make_batch(spec, batch=2, frames=2, audio_slices=1, txt_len=16, seed=6)
    decode.generate_cap(m, batch, ["tv"], mode="sample", seed=3)
    decode.release_sessions(m)
    assert any(cap for cap, _ in seen), seen                              # a step was captured ...
    assert all(on != cap for cap, on in seen), seen                        # ... with the collector off exactly there
    assert gc.isenabled()
