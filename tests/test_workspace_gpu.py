"""The per-stream scratch buffers of `hip.ops._workspace`: reuse on one stream, separation between streams, and results
that do not depend on how large the buffer has grown (some calls size their split-K slabs by the room they are given)."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def test_large_workspaces_are_reused_per_stream_and_results_do_not_depend_on_their_size():
    from onnx_quantize_amd.hip import ops

    ops.release_workspaces()
    dev = torch.device("cuda", 0)
    a = ops._workspace(64 << 20, dev)
    b = ops._workspace(48 << 20, dev)
    assert a.data_ptr() == b.data_ptr() and b.numel() == 48 << 20          # same buffer, exactly the bytes asked for
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        c = ops._workspace(64 << 20, dev)
    assert c.data_ptr() != a.data_ptr()                                     # another stream never shares it
    small1, small2 = ops._workspace(4096, dev), ops._workspace(4096, dev)
    assert small1.data_ptr() != small2.data_ptr()                           # small requests are ordinary allocations

    g = torch.Generator(device=dev).manual_seed(5)
    x = torch.randn((4, 2048, 4096), generator=g, device=dev)
    ops.release_workspaces()
    h1 = torch.zeros((4096, 4096), device=dev)
    ops.hessian_accumulate(x, h1, 0)
    ops._workspace(3 << 30, dev)                                            # grow the buffer far beyond what the call needs
    h2 = torch.zeros((4096, 4096), device=dev)
    ops.hessian_accumulate(x, h2, 0)
    assert torch.equal(h1, h2)
    ops.release_workspaces()
    assert not ops._ARENA
    # a caller cycling through many streams does not pin one buffer per stream
    streams = [torch.cuda.Stream(device=dev) for _ in range(ops._ARENA_MAX_STREAMS + 3)]
    for s_ in streams:
        with torch.cuda.stream(s_):
            ops._workspace(40 << 20, dev)
    assert len(ops._ARENA) == ops._ARENA_MAX_STREAMS
    assert (0, streams[-1].cuda_stream) in ops._ARENA and (0, streams[0].cuda_stream) not in ops._ARENA
    ops.release_workspaces()


def test_the_minmax_workspace_is_kept_for_at_most_four_streams():
    from onnx_quantize_amd.hip import ops

    ops.release_workspaces()
    dev = torch.device("cuda", 0)
    x = torch.randn((1, 64), generator=torch.Generator(device=dev).manual_seed(7), device=dev)
    streams = [torch.cuda.Stream(device=dev) for _ in range(ops._ARENA_MAX_STREAMS + 2)]
    states = [ops.minmax_state(dev) for _ in streams]
    torch.cuda.synchronize()                                                # x and the states are ready for every stream
    for s_, state in zip(streams, states):
        with torch.cuda.stream(s_):
            ops.minmax_collect(x, state)
    torch.cuda.synchronize()
    assert len(ops._MINMAX_WS) == ops._ARENA_MAX_STREAMS
    assert (0, streams[-1].cuda_stream) in ops._MINMAX_WS and (0, streams[0].cuda_stream) not in ops._MINMAX_WS
    for state in states:                                                    # an evicted workspace took no result with it
        assert state[0] == x.min() and state[1] == x.max()
    ops.release_workspaces()
    assert not ops._MINMAX_WS


def test_the_rtn_state_is_kept_for_at_most_four_streams_and_comes_back_zeroed():
    from onnx_quantize_amd.hip import ops

    ops.release_workspaces()
    dev = torch.device("cuda", 0)
    streams = [torch.cuda.Stream(device=dev) for _ in range(ops._ARENA_MAX_STREAMS + 2)]
    with torch.cuda.stream(streams[0]):
        ops._rtn_state(1, dev).fill_(1)                                     # whatever block comes back after the eviction, not these bytes
    for s_ in streams[1:]:
        with torch.cuda.stream(s_):
            last = ops._rtn_state(1, dev)
    assert 0 < len(ops._RTN_STATE) <= ops._ARENA_MAX_STREAMS
    assert (0, streams[0].cuda_stream) not in ops._RTN_STATE
    with torch.cuda.stream(streams[-1]):
        again = ops._rtn_state(1, dev)
    assert again.data_ptr() == last.data_ptr() and again.numel() == last.numel() >= 1 << 20      # the whole buffer, the same one
    with torch.cuda.stream(streams[0]):
        back = ops._rtn_state(1, dev)                                       # evicted above: a NEW zero-filled buffer
        assert back.numel() >= 1 << 20 and not back.any()
    ops.release_workspaces()
    assert not ops._RTN_STATE
