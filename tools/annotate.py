"""Annotate the images of a directory: the loop of the reference's ``demo.py --img_dir`` without a window.

Every ``*.jpg`` / ``*.jpeg`` / ``*.png`` of the directory is read (``FaceAna.imread``: baseline JPEG is decoded on the GPU), run
through ``FaceAna.run`` and ``reset`` -- no tracking from one file to the next, as in the demo -- and the frame with a dot on each of
the 98 landmarks, white where the score exceeds 0.8 and red elsewhere, is written next to the input as ``<name>.annotated.jpg``.  The
overlay and the JPEG encoder run on the GPU (``draw`` and ``jpeg`` options of FaceAna), so only the file leaves the device.

    python tools/annotate.py DIR [--what points contours box] [--radius 2] [--width 1] [--alpha 256] [--quality 90] [--redact]
"""
from __future__ import annotations

import argparse
import os
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SUFFIX = ".annotated.jpg"


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("img_dir")
    ap.add_argument("--what", nargs="+", default=["points"], choices=["points", "contours", "box"])
    ap.add_argument("--radius", type=int, default=2, help="point radius in pixels (1..16)")
    ap.add_argument("--width", type=int, default=1, help="line width of contours and box in pixels (1..16)")
    ap.add_argument("--alpha", type=int, default=256, help="1..256, 256 = opaque")
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--redact", action="store_true", help="pixelate the faces first and draw over the redaction")
    return ap.parse_args(argv)


def annotate(facer, img_dir):
    """-> [(input path, output path or None when the file could not be read, faces, seconds)]"""
    done = []
    names = sorted(n for n in os.listdir(img_dir)
                   if n.lower().endswith((".jpg", ".jpeg", ".png")) and not n.endswith(SUFFIX))
    for name in names:
        path = os.path.join(img_dir, name)
        image = facer.imread(path, want_host=False)
        if image is None:
            done.append((path, None, 0, 0.0))
            continue
        t0 = time.time()
        result = facer.run(image)
        facer.reset()                                    # no tracking between files
        out = os.path.splitext(path)[0] + SUFFIX
        with open(out, "wb") as f:
            f.write(facer.last_drawn_jpeg)
        done.append((path, out, len(result), time.time() - t0))
    return done


def main(argv=None):
    args = parse_args(argv)
    from Skps import FaceAna
    draw = {"what": tuple(args.what), "point_radius": args.radius, "line_width": args.width, "alpha": args.alpha}
    redact = None
    if args.redact:
        redact, draw["base"] = {"mode": "mosaic", "strength": 16}, "redacted"
    facer = FaceAna(draw=draw, redact=redact, jpeg={"quality": args.quality, "raw": False})
    for path, out, faces, s in annotate(facer, args.img_dir):
        if out is None:
            print("%s: cannot be read" % path)
        else:
            print("%s -> %s: %d faces, %.3f s" % (path, out, faces, s))


if __name__ == "__main__":
    main()
