"""Langevin samplers and online statistics (mirrors reference ``pyxu.experimental.sampler``)."""
from pyxu_amd.experimental.sampler._sampler import *  # noqa: F401,F403
from pyxu_amd.experimental.sampler.statistics import *  # noqa: F401,F403
