"""Command line of the encoder: starts the native program (wrenc_amd/csrc/host/wrenc, built by build()) with the same
arguments, so that `python -m wrenc_amd.cli` and the program are one pipeline.

    python -m wrenc_amd.cli -i in.yuv -o out.vvc --input-size 1920x1088 --output-size 1920x1088 \
        --num-pictures 30 --qp 32 --max-split-depth 2 [--reconst rec.yuv]

The program takes the reference's options (main.rs:85-115) and a few of its own (README; among them --pad, with which
--output-size may be any even size such as 1920x1080, and --hash md5|crc|checksum, which puts a decoded picture hash SEI
behind every slice, and --input-format rgb24|bgr24|rgb0|bgr0|rgba|bgra|gbrp with --colorspace bt709|bt601 and --range tv|pc
for RGB frames, which the device converts); its standard streams are
this process's and its exit status is this one's: 0 on success and, like the reference, on argument and I/O errors
(main.rs:127-133); 101 where the reference panics.  There is no CPU path: without an MI355X the command fails.
"""
import os
import subprocess
import sys

NATIVE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "host", "wrenc")


def main(argv=None):
    if not os.path.exists(NATIVE):
        sys.stderr.write("error: %s is missing: run `python -c 'import __graft_entry__ as g; g.build()'`\n" % NATIVE)
        return 101
    rc = subprocess.run([NATIVE] + list(sys.argv[1:] if argv is None else argv)).returncode
    return rc if rc >= 0 else 128 - rc     # killed by a signal: the shell's status for it


if __name__ == "__main__":
    sys.exit(main())
