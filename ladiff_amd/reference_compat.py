"""Makes the reference's loop-owner import resolve to this package, with no edit to the reference.

The reference finds its model class by name: `get_module` (`src/ladiff/models/get_model.py:12-17`) runs
`importlib.import_module(".modeltype.ladiff", package="ladiff.models")` and takes its `LADIFF`.  `install()` redirects that one
dotted name, `ladiff.models.modeltype.ladiff`, to a module whose `LADIFF` is `ladiff_amd.pipeline.LADIFF`; every other name under
`ladiff.*` (datamodules, configs, transforms, ...) stays the reference's.  It works whether or not the reference's packages are
already imported: a finder at the front of `sys.meta_path` serves later imports, and an entry already in `sys.modules` is replaced.

    python -m ladiff_amd.reference_compat demo.py --cfg ... --example ...

runs a script of the reference unchanged, in this process, after `install()`.  `demo.py:182` then finds
`LADIFF.forward_motion_style_transfer(batch)`, which the reference's own class lacks: here it is `LADIFF.edit(batch, strength=
model.demo_strength or 0.6)` - SDEdit, not MLD's three-branch guidance.
"""
import importlib.abc
import importlib.util
import os
import runpy
import sys

TARGET = "ladiff.models.modeltype.ladiff"


class _LoopOwnerFinder(importlib.abc.MetaPathFinder, importlib.abc.Loader):
    """Finds and loads `TARGET` only; returns None (the normal search) for every other name."""

    def find_spec(self, fullname, path=None, target=None):
        if fullname != TARGET:
            return None
        return importlib.util.spec_from_loader(fullname, self)

    def create_module(self, spec):
        return None                      # the default module object

    def exec_module(self, module):
        from ladiff_amd.pipeline import LADIFF
        module.LADIFF = LADIFF
        module.__all__ = ["LADIFF"]


_FINDER = _LoopOwnerFinder()


def install():
    """Redirect `ladiff.models.modeltype.ladiff` to a module holding `ladiff_amd.pipeline.LADIFF`.  Idempotent."""
    if _FINDER not in sys.meta_path:
        sys.meta_path.insert(0, _FINDER)
    current = sys.modules.get(TARGET)
    if current is not None and getattr(current, "__loader__", None) is _FINDER:
        return current
    if current is not None or TARGET.rpartition(".")[0] in sys.modules:
        # imported already (or its package is): replace the entry and the package attribute that `from ... import ladiff` reads
        spec = _FINDER.find_spec(TARGET)
        module = importlib.util.module_from_spec(spec)
        _FINDER.exec_module(module)
        sys.modules[TARGET] = module
        parent = sys.modules.get(TARGET.rpartition(".")[0])
        if parent is not None:
            setattr(parent, TARGET.rpartition(".")[2], module)
        return module
    return None


def main(argv=None):
    """`python -m ladiff_amd.reference_compat SCRIPT [args...]`: install(), then run SCRIPT as `__main__` in this process with
    sys.argv = [SCRIPT, args...] and the script's directory first on sys.path, as `python SCRIPT args...` would."""
    argv = list(sys.argv[1:] if argv is None else argv)
    if not argv or argv[0] in ("-h", "--help"):
        print("usage: python -m ladiff_amd.reference_compat SCRIPT [args...]", file=sys.stderr)
        return 2
    script = argv[0]
    install()
    sys.argv = [script] + argv[1:]
    sys.path.insert(0, os.path.dirname(os.path.abspath(script)))
    runpy.run_path(script, run_name="__main__")
    return 0


if __name__ == "__main__":
    sys.exit(main())
