"""The refusals ModelMemory.anchor_reports / anchor_claims / anchor_bank_audit share (memvul_amd/kept_sweep.py KeptSweepState states them once), on the
oracle-backed stand-in: each of the three must give every one of them under its own name, before any index is built."""
import re

import pytest

from kept_index_kit import _NumpyBank, _NumpyClaims, _NumpyIndex, standin_model  # noqa: F401  (standin_model is a fixture)

TOOLS = {"reports": ("anchor_reports", (5,), _NumpyIndex), "claims": ("anchor_claims", (0.5,), _NumpyClaims), "bank": ("anchor_bank_audit", (0.5,), _NumpyBank)}


@pytest.mark.parametrize("kind", list(TOOLS))
def test_the_shared_refusals(standin_model, kind):
    model, arrays, _ = standin_model
    who, args, factory = TOOLS[kind]

    def ask(**kw):
        return getattr(model, who)(arrays, *args, index_factory=factory, **kw)

    no_sweep = re.escape(f"{who}(): no kept sweep of these rows — call sweep_arrays(arrays, first, last, keep=True) first (the resident corpus keeps")
    with pytest.raises(RuntimeError, match=no_sweep):
        ask()
    model.sweep_arrays(arrays, batch_size=8, with_probs=True)  # not a keeping sweep
    with pytest.raises(RuntimeError, match=no_sweep):
        ask()
    model.sweep_arrays(arrays, batch_size=8, keep=True)
    with pytest.raises(RuntimeError, match=no_sweep):
        ask(first=0, last=10)  # other rows than the kept sweep's
    if kind == "bank":  # (it audits the bank alone: its labels are the golden labels)
        labels, model._golden_labels = model._golden_labels, model._golden_labels[:3]
        with pytest.raises(ValueError, match=re.escape(f"{who}(): 3 labels for 4 anchors")):
            ask()
        model._golden_labels = labels
    else:
        with pytest.raises(ValueError, match=re.escape(f"{who}(): 1 labels for 2 vectors")):
            ask(vectors=model.engine.anchor_get()[[2, 0]], labels=["one"])
    weight, model._kept.matcher_weight = model._kept.matcher_weight, None  # (what load_state_dict leaves when the state dict has no matcher)
    with pytest.raises(RuntimeError, match=re.escape(f"{who}(): the state dict held no _projector.weight")):
        ask()
    assert factory.made == [] and model._kept.indexes == dict.fromkeys(("reports", "claims", "bank", "ranking")) and model._kept.embed is None
    model._kept.matcher_weight = weight
    ask()
    assert len(factory.made) == 1 and model._kept.indexes[kind] is factory.made[0]
    ask()
    assert len(factory.made) == 1
