"""Experimental components (mirrors reference ``pyxu.experimental``): ``sampler``."""
