"""asvspoof2021_air_amd -- MI355X-native hot path of yzyouzhang/ASVspoof2021_AIR.

LFCC front-end -> ResNet / ECAPA-TDNN forward+backward -> OC-Softmax (ang_iso),
behind the reference's Python module surface:

    from asvspoof2021_air_amd.feature_extraction import LFCC
    from asvspoof2021_air_amd.resnet import ResNet
    from asvspoof2021_air_amd.loss import AngularIsoLoss, OCSoftmax

All device arithmetic runs in hand-written gfx950 HIP kernels reached through
the C-ABI in include/air_hip.h (libair_hip.so, loaded with ctypes).

The GMM back-end (gmm.py) is exported here: ``from asvspoof2021_air_amd import DiagGMM, GMMBackend``, and so is the
CQCC front-end (feature_extraction.py): ``from asvspoof2021_air_amd import CQCC``.
"""
__version__ = "0.1.0"


def __getattr__(name):  # resolved on first use: importing the package stays as light as it was
    if name in ("DiagGMM", "GMMBackend"):
        from . import gmm
        return getattr(gmm, name)
    if name == "CQCC":
        from . import feature_extraction
        return feature_extraction.CQCC
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
