"""The one fixture factory for test modules that move the library's process-wide training switches
(``rag4dyg_amd.training.TRAIN_MODE_AXES``: every ``r4d_set_train_*``), and a helper for tests that ask whether an entry point takes a
mode keyword.  A switch that a failing test left on would change what every later module measures; the fixture puts back ALL of
them, whatever the module itself touches -- a new switch is covered by its table row, not by an edit here."""
import argparse
import inspect
import os

import pytest

TOOLS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")


def switches_restored(ops_too=False, force_stored=()):
    """An autouse fixture: after every test all training switches are what they were before it.  ``ops_too``: the encoder's
    ``ops.encode_precision()`` and ``ops.gemm_mode()`` as well.  ``force_stored``: of ``"attention"`` / ``"activations"``, the
    switches that end at 0 (stored) whatever they were -- the modules that promise the later ones the default."""
    @pytest.fixture(autouse=True)
    def _switches_restored():
        from rag4dyg_amd import _lib, ops, training
        was_ops = (ops.encode_precision(), ops.gemm_mode()) if ops_too else None
        with training.saved_library_modes():
            yield
        for switch in force_stored:
            _lib.check(getattr(_lib.load(), "r4d_set_train_" + switch)(0), "set_train_" + switch)
        if ops_too:
            ops.set_encode_precision(was_ops[0])
            ops.set_gemm_mode(was_ops[1])
    return _switches_restored


def takes_mode_keyword(fn, key):
    """Whether ``fn`` (a trainer's ``__init__`` or a ``train()``) takes the mode keyword ``key`` with None as its default: named in
    the signature, or through ``**modes`` -- then ``key`` must be an axis of the table, which :meth:`TrainModes.resolve` opens."""
    from rag4dyg_amd import training
    params = inspect.signature(fn).parameters
    if key in params:
        return params[key].default is None
    through_modes = "modes" in params and params["modes"].kind is inspect.Parameter.VAR_KEYWORD
    return through_modes and key in [a.key for a in training.TRAIN_MODE_AXES]


def tool_mode_choices(tool, flag):
    """(text of ``tools/<tool>``, the words it accepts for the training-mode option ``flag``).  The tools take these options from
    the table -- ``training.add_mode_arguments(parser)``, or a loop over ``TRAIN_MODE_AXES`` --, so the words are read where the tool
    reads them; None for a tool that does neither, or a flag that is no axis."""
    from rag4dyg_amd import training
    text = open(os.path.join(TOOLS, tool)).read()
    if "add_mode_arguments(" not in text and "TRAIN_MODE_AXES" not in text:
        return text, None
    ap = argparse.ArgumentParser()
    training.add_mode_arguments(ap)
    return text, next((tuple(a.choices) for a in ap._actions if flag in a.option_strings), None)
