"""The buffer model's bucket walked over a stream's own bytes (include/wrenc_rate.h): the stream is split into its
parameter sets and its pictures -- a picture is its picture header NAL unit and everything up to the next one: the slice
and, with --hash, the SEI -- and nothing the program reports is read."""
from window_stream import PREFIX, split_raw

NAL_PH = 19


def picture_bytes(stream):
    """(bytes of the parameter sets, [bytes of every picture]), prefixes included: together the whole stream."""
    header, pictures = 0, []
    for unit in split_raw(stream):
        size = len(PREFIX) + len(unit)
        if unit[1] >> 3 == NAL_PH:
            pictures.append(size)
        elif pictures:
            pictures[-1] += size
        else:
            header += size
    assert header + sum(pictures) == len(stream)
    return header, pictures


def walk(stream, bufsize_bits, bits_per_picture):
    """F_0 = B; picture i takes bits_i out of F_i (the parameter sets count to picture 0); F_(i+1) = min(B, F_i - bits_i + R).
    Returns {"left": [F_i - bits_i], "violations": [i with bits_i > F_i]}."""
    header, pictures = picture_bytes(stream)
    fullness, left, violations = float(bufsize_bits), [], []
    for i, size in enumerate(pictures):
        bits = 8.0 * (size + (header if i == 0 else 0))
        left.append(fullness - bits)
        if bits > fullness:
            violations.append(i)
        fullness = min(float(bufsize_bits), fullness - bits + bits_per_picture)
    return {"left": left, "violations": violations}
