"""Drop-in alias: ``from Skps import FaceAna`` keeps working (reference Skps/__init__.py:7-9); ``StreamTracker`` tracks N
camera feeds on one engine."""
from peppa_pig_face_landmark_amd.core.api.facer import FaceAna
from peppa_pig_face_landmark_amd.core.api.stream_tracker import StreamTracker

__all__ = ["FaceAna", "StreamTracker"]
