"""Every cached weight image, engine and graph plan is held to the live parameters (tests/coherence.py is the harness).

The kernels are held to fp64 models elsewhere; none of them reads a Parameter. They read the weight images, and captured graphs read
them - and the variance - through raw pointers. A cache that goes stale leaves every kernel bit-exact on the wrong weights: nothing
faults, nothing turns NaN. So:

  control  with no route applied, every consumer on a renderer equals the same consumer on its twin (a renderer freshly built from
           its state_dict) bit for bit, in bf16 and in fp32 - the comparison itself has no slack;
  matrix   ROUTES x precision: every consumer once (images, engines, graph plans, scratch buffers exist), the route, every consumer
           again, and the result against the twin built after the route, bit for bit; and the outputs must have moved - a route
           that changes nothing observable proves nothing;
  teeth    with NetImages.refresh made to skip every rebuild after the first, the `inplace` cell must fail; with refresh_together
           skipped, the `trainer_step` cell must.

Sizes: 64 and 77 rays (a ragged last workgroup) of 128 + 32 samples, 300 points, a 16^3 lattice - the smallest that reach every
launch variant the consumers have; a cell builds one renderer and its twins."""
import pytest
import torch

import coherence as co

pytestmark = pytest.mark.gpu

# consumer -> max |a - b| allowed against the twin, for a consumer whose control is NOT bit-identical (4 x the control's own
# difference, measured and written down here). Empty: every consumer's control is bit-identical.
CONTROL_TOL = {}


@pytest.fixture(autouse=True)
def _harness_objects():
    keep = []
    yield keep
    keep.clear()
    co.forget()


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_control_renderer_equals_its_twin(precision, _harness_objects):
    """No route: a renderer with all its caches built equals its twin, every consumer, bit for bit - twice (the second round runs
    on warm caches and replayed graphs on both sides)."""
    rend = co.make(precision)
    tw = co.twin(rend)
    _harness_objects += [rend, tw]
    for round_ in range(2):
        a, b = co.consume(rend), co.consume(tw)
        bad = co.differing(a, b)
        for c in sorted({c for c, _ in bad}):
            print("control %s round %d: %s differs from the twin by max |a - b| = %.3e" % (precision, round_, c, co.max_abs_diff(a, b, c)))
        assert not bad, (round_, bad[:8])
        assert all(torch.isfinite(t).all() for c in a for t in a[c].values())


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
@pytest.mark.parametrize("route", list(co.ROUTES))
def test_route_leaves_every_consumer_on_the_live_weights(route, precision, _harness_objects):
    co.run_cell(route, precision, tol=CONTROL_TOL, keep=_harness_objects)


def test_teeth_a_skipped_image_rebuild_is_caught(monkeypatch, _harness_objects):
    """NetImages.refresh rebuilds once and never again: the `inplace` cell - versions bumped, nothing rebuilt - must fail on its
    comparison with the twin."""
    from vdn_hip import images
    real = images.NetImages.refresh

    def once(self, stream):
        if self.__dict__.get("_built_once"):
            return False
        self.__dict__["_built_once"] = True
        return real(self, stream)
    monkeypatch.setattr(images.NetImages, "refresh", once)
    with pytest.raises(AssertionError, match=r"differ from its twin.*\('render_nograd', 'color_fine'\)"):
        co.run_cell("inplace", "bf16", keep=_harness_objects)


def test_teeth_a_skipped_refresh_together_is_caught(monkeypatch, _harness_objects):
    """refresh_together does nothing: the Trainer's raw-pointer Adam moves the weights, no version counter moves, nothing rebuilds the
    images - the `trainer_step` cell must fail on its comparison with the twin."""
    from vdn_hip import images
    monkeypatch.setattr(images, "refresh_together", lambda ims, stream, cache: None)
    with pytest.raises(AssertionError, match=r"differ from its twin.*\('render_nograd', 'color_fine'\)"):
        co.run_cell("trainer_step", "bf16", keep=_harness_objects)
