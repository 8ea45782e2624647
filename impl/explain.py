"""Module `impl.explain` (an extension: the reference has none): edge saliency and learned edge masks, backed by
glass_amd.explain (MI355X HIP path)."""
import sys as _sys

from glass_amd import explain as _impl

_sys.modules[__name__] = _impl
