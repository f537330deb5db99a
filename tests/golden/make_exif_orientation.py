"""Writes tests/golden/exif_orientation.json: EXIF payloads, as PictureMetadata.exif / sjpeg_hip_metadata.exif take them,
and the Orientation (IFD0 tag 0x0112) a reader has to find in each -- 0 where there is none to find.  The big-endian
payloads are Pillow's (Image.Exif.tobytes(): "Exif\\0\\0", "MM", IFD0); the little-endian ones are the same IFDs
written out here byte by byte, with and without the "Exif\\0\\0" in front.  Only this generator uses Pillow; the tests
(tests/test_orient_host.py, tests/cxx/exif_orientation_test.cc through tests/test_exif_orientation_cxx.py) read the JSON.

Every case: {"name", "hex": the payload, "orientation": 0..8, "reset_hex": the payload after
sjpeg_hip_exif_reset_orientation (equal to "hex" where orientation is 0)}.

    python tests/golden/make_exif_orientation.py
"""
import json
import os
import struct

from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "exif_orientation.json")


def pillow(tags):
    e = Image.Exif()
    for k, v in tags:
        e[k] = v
    return e.tobytes()


def little(entries, prefix=True, next_ifd=0):
    """A little-endian TIFF block with one IFD at offset 8: entries = [(tag, type, count, 4 value bytes)]"""
    b = b"II" + struct.pack("<HI", 42, 8) + struct.pack("<H", len(entries))
    for tag, typ, count, value in entries:
        b += struct.pack("<HHI", tag, typ, count) + value
    b += struct.pack("<I", next_ifd)
    return (b"Exif\0\0" if prefix else b"") + b


def short(v, big=False):
    return struct.pack(">HH" if big else "<HH", v, 0)


def reset(payload, big, value_at):
    """the payload with the SHORT at value_at set to 1"""
    return payload[:value_at] + struct.pack(">H" if big else "<H", 1) + payload[value_at + 2:]


def main():
    cases = []

    def add(name, payload, orientation, value_at=None, big=False):
        after = payload if orientation == 0 else reset(payload, big, value_at)
        cases.append(dict(name=name, hex=payload.hex(), orientation=orientation, reset_hex=after.hex()))

    for o in range(1, 9):
        p = pillow([(0x0112, o)])
        assert p[:6] == b"Exif\0\0" and p[6:8] == b"MM" and p[16:18] == b"\x01\x12"
        add("pillow big-endian %d" % o, p, o, 6 + 8 + 2 + 8, True)
        add("little-endian %d" % o, little([(0x0112, 3, 1, short(o))]), o, 6 + 8 + 2 + 8)
    # no "Exif\0\0" in front: the TIFF header comes first
    add("little-endian 6, TIFF header first", little([(0x0112, 3, 1, short(6))], prefix=False), 6, 8 + 2 + 8)
    add("pillow big-endian 8, TIFF header first", pillow([(0x0112, 8)])[6:], 8, 8 + 2 + 8, True)
    # the tag behind other IFD0 tags (Make, in front; Software, behind: their strings lie behind the IFD)
    p = pillow([(0x010F, "Maker"), (0x0112, 8), (0x0131, "soft")])
    assert p[6 + 10:6 + 12] == b"\x01\x0f" and p[6 + 22:6 + 24] == b"\x01\x12"
    add("pillow big-endian 8 behind Make", p, 8, 6 + 8 + 2 + 12 + 8, True)
    add("little-endian 3 behind two tags",
        little([(0x0100, 4, 1, struct.pack("<I", 4000)), (0x0101, 4, 1, struct.pack("<I", 3000)), (0x0112, 3, 1, short(3))]), 3,
        6 + 8 + 2 + 24 + 8)
    # nothing to find
    add("pillow big-endian, no Orientation", pillow([(0x010F, "Maker"), (0x0131, "soft")]), 0)
    add("little-endian, no Orientation", little([(0x0100, 4, 1, struct.pack("<I", 4000))]), 0)
    add("little-endian, type LONG", little([(0x0112, 4, 1, struct.pack("<I", 6))]), 0)
    add("big-endian, type LONG", b"Exif\0\0MM" + struct.pack(">HIH", 42, 8, 1) + struct.pack(">HHII", 0x0112, 4, 1, 6) + b"\0" * 4, 0)
    add("little-endian, count 2", little([(0x0112, 3, 2, struct.pack("<HH", 6, 6))]), 0)
    add("little-endian, value 0", little([(0x0112, 3, 1, short(0))]), 0)
    add("little-endian, value 9", little([(0x0112, 3, 1, short(9))]), 0)
    add("little-endian, IFD0 offset past the end", b"Exif\0\0II" + struct.pack("<HI", 42, 4000), 0)
    add("bad magic", b"Exif\0\0II" + struct.pack("<HI", 43, 8) + struct.pack("<H", 0), 0)
    add("not TIFF", b"Exif\0\0JFIF and then some bytes", 0)
    add("empty", b"", 0)
    add("prefix only", b"Exif\0\0", 0)
    add("entry count larger than the block", b"Exif\0\0II" + struct.pack("<HIH", 42, 8, 9) + struct.pack("<HHII", 0x0100, 4, 1, 1), 0)
    # a next-IFD offset past the end is not followed: IFD0's tag is found all the same
    add("little-endian 5, next IFD past the end", little([(0x0112, 3, 1, short(5))], next_ifd=0x7fffff00), 5, 6 + 8 + 2 + 8)
    with open(OUT, "w") as f:
        json.dump(dict(comment="EXIF payloads and their Orientation; made by make_exif_orientation.py (Pillow %s)" %
                       __import__("PIL").__version__, cases=cases), f, indent=1)
        f.write("\n")
    print("%d cases -> %s" % (len(cases), OUT))


if __name__ == "__main__":
    main()
