"""Drop-in alias: `remfx.effects` -> `remfx_amd.effects` (every effect class of the reference's remfx/effects.py, RandomSoxReverb
included, the biqaud / parametric_eq / stereo_widener helpers, LoudnessNormalize, RandomAudioEffectsChannel and the
Pedalboard_Effects label order) so that cfg/effects/all.yaml's `_target_` strings and `from remfx.effects import ...` lines
resolve to the MI355X build."""
from remfx_amd.effects import *  # noqa: F401,F403
from remfx_amd import effects as _impl

__all__ = [n for n in dir(_impl) if not n.startswith("__")]
globals().update({n: getattr(_impl, n) for n in dir(_impl) if not n.startswith("__")})
