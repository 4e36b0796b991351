"""A native object that owns device memory (Go1Sim, Go1Reward: their destroy calls hipFree) is released by `go1sim_host.release`, which puts
the destroy off while the releasing thread's stream is being captured: a hipFree inside a capture invalidates the capture, and an
environment is part of reference cycles, so it is the garbage collector that releases it, wherever it happens to run."""
import gc
import weakref

import pytest
import torch


def test_release_is_put_off_during_a_capture_and_made_up_for_after_it(monkeypatch):
    import go1sim_host as H
    import go1reward_host as R
    assert R.release is H.release and H._PUT_OFF == []
    done = []
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    H.release(done.append, 11)
    H.release(done.append, 12)
    assert done == [] and [h for _, h in H._PUT_OFF] == [11, 12]
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    H.release(done.append, 13)                                            # outside a capture: what was put off goes first
    assert sorted(done[:2]) == [11, 12] and done[2] == 13 and H._PUT_OFF == []
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)        # without a GPU nothing is asked about a capture
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: pytest.fail("asked"))
    H.release(done.append, 14)
    assert done[3] == 14

    class Owner:                                                          # the two destructors go through it and swallow what it raises
        handle, lib = 5, None
    for cls, name in ((H.Go1Sim, "go1sim_destroy"), (R.Go1Reward, "go1reward_destroy")):
        owner = Owner()
        owner.lib = type("Lib", (), {name: staticmethod(done.append)})
        cls.__del__(owner)
        assert done[-1] == 5 and owner.handle is None
        cls.__del__(owner)
        assert done.count(5) == len(done) - 4


@pytest.mark.gpu
def test_an_environment_collected_inside_a_stream_capture_leaves_the_capture_whole():
    """an environment dropped before a capture and collected inside it (the collector is called there on purpose; in the suite it runs when
    it runs): the capture ends whole and replays, the simulator's destroy is put off and made up for by the next release"""
    import go1sim_host as H
    from test_gpu_response_trace import DEVICE, make_env
    env = make_env(16, "plane", 20.0)
    env.step(torch.zeros(16, 12, device=DEVICE))
    alive = weakref.ref(env.sim)
    x = torch.zeros(64, device=DEVICE)
    torch.cuda.synchronize()
    gc.collect()
    gc.disable()
    try:
        del env                                                           # part of reference cycles: only the collector releases it
        assert alive() is not None and H._PUT_OFF == []
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            gc.collect()
            y = x + 1.0
    finally:
        gc.enable()
    assert alive() is None and len(H._PUT_OFF) == 1
    graph.replay()
    torch.cuda.synchronize()
    assert bool((y == 1.0).all())
    H.release(lambda handle: None, None)
    assert H._PUT_OFF == []
