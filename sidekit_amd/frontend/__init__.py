"""``sidekit.frontend``: the part of the reference's front-end package the speech-only extraction path needs (``vad_energy`` lives in
``sidekit.mixture`` and, identically, in ``sidekit.frontend.vad``; ``label_fusion`` in ``sidekit.frontend.vad``)."""
from .vad import label_fusion, vad_energy  # noqa: F401
