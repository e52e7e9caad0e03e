"""Drop-in for the reference's `model.classifier` import path (eval/main_classifier.py:26):
re-exports the MI355X-native implementation."""
from coclr_amd.model.classifier import LinearClassifier  # noqa: F401

# eval/main_classifier.py:157-159 construct `optim.Adam` / `optim.SGD` over one param group per tensor:
# resolve them to the single-launch subclasses (COCLR_PATCH_ADAM=0 / COCLR_PATCH_SGD=0 keep torch's).
from coclr_amd import optim as _optim  # noqa: E402
_optim.install()
