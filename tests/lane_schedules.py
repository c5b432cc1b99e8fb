"""Four-lane schedules for the small GPU scenes — TEST INFRASTRUCTURE.

With four lanes and a caller's stream, lane 0 leaves the caller's stream for the context's own
(pbr_kernels.hip wf_fork): the fork waits on lane 0 too, the join and the per-frame events record on
it.  That is the default of every full-size Path frame, so the small tests run it on purpose, in the
three regimes the render loops treat differently:

- more chunks than lanes (fork and join per frame, the lanes' buffers reused chunk after chunk);
- fewer chunks than lanes (a batch's frames and passes continue one rotation over the lanes);
- 24 or more chunks, balanced to a whole number per lane.

Which regime a chunk_log2 lands in depends on the frame's samples, so every test states the regime it
means and checks it against what the device ran (HipRenderer.last_chunks): a scene-size change cannot
move a case out of its regime unnoticed."""

MORE, ROTATING, BALANCED = "more_chunks_than_lanes", "fewer_chunks_than_lanes", "balanced_24_or_more"


def four_lanes(more, rotating, balanced):
    """name → (set_schedule arguments, regime) for the chunk_log2 of each regime."""
    return {"l4_more_chunks": ({"chunk_log2": more, "lanes": 4}, MORE),
            "l4_rotating": ({"chunk_log2": rotating, "lanes": 4}, ROTATING),
            "l4_balanced": ({"chunk_log2": balanced, "lanes": 4}, BALANCED)}


def assert_regime(plan, regime, caller_stream, batch):
    """`plan` (last_chunks of the call just queued) is in `regime` on four lanes, lane 0 on the
    context's stream exactly when the call came on a caller's stream."""
    n, lanes = plan["n_chunks"], plan["lanes"]
    if regime == MORE:
        assert lanes == 4 and 4 < n < 24, plan
    elif regime == ROTATING:
        # (a single frame of one chunk runs on one lane; a batch keeps the lanes and rotates)
        assert 1 <= n < 4 and lanes == (4 if batch or n > 1 else 1), plan
    else:
        assert lanes == 4 and n >= 24 and n % 4 == 0, plan
    assert plan["lane0_on_ctx_stream"] == (bool(caller_stream) and lanes == 4), plan
