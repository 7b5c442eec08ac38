"""``sidekit.frontend``: the part of the reference's front-end package that is built.

For the speech-only extraction path: ``vad_energy`` (it lives in ``sidekit.mixture`` and, identically, in ``sidekit.frontend.vad``) and
``label_fusion`` (``sidekit.frontend.vad``).  For the feature post-processing: ``rasta_filt``, ``cms``, ``cmvn``, ``stg`` and
``cep_sliding_norm`` (``sidekit.frontend.normfeat``) and ``compute_delta`` (``sidekit.frontend.features``).  For the cepstral front end:
``mfcc``, ``power_spectrum``, ``trfbank``, ``hz2mel``, ``mel2hz`` and ``dct_basis`` (``sidekit.frontend.features``)."""
from .vad import label_fusion, vad_energy  # noqa: F401
from .features import compute_delta, dct_basis, hz2mel, mel2hz, mfcc, pca_dct, power_spectrum, shifted_delta_cepstral, trfbank  # noqa: F401
from .normfeat import cep_sliding_norm, cms, cmvn, rasta_filt, stg  # noqa: F401
