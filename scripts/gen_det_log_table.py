"""Print the table and constants of csrc/det_log.hpp (stdlib only: decimal at 80 digits).

det_log reduces x = 2^k z with z in [0.6875, 1.375) and looks z's top 7 mantissa bits up (as the bit pattern of
z minus that of 0.6875 is cut): entry i covers the doubles with patterns [OFF + i 2^45, OFF + (i + 1) 2^45), has
invc = RN(1 / centre) and the double-double (logc_hi, logc_lo) = -log(invc), so that
log(z) = -log(invc) + log1p(z invc - 1) holds exactly for the tabulated invc, whatever its rounding.  The two entries
next to 1 (i = 79: [1 - 2^-8, 1), i = 80: [1, 1 + 2^-7)) have invc = 1, logc = 0: there z invc - 1 = z - 1 is exact.

    python scripts/gen_det_log_table.py > /tmp/table.inc     # paste between the markers of det_log.hpp
"""
import struct
from decimal import Decimal, getcontext

getcontext().prec = 80
OFF = 0x3FE6000000000000
N = 128


def dbl(bits):
    return struct.unpack("<d", struct.pack("<Q", bits))[0]


def rn(d):
    """Decimal -> nearest double (float() of a decimal string is correctly rounded)."""
    return float(str(d))


def dd(d):
    hi = rn(d)
    return hi, rn(d - Decimal(hi))


def entries():
    out = []
    for i in range(N):
        lo, hi = dbl(OFF + (i << 45)), dbl(OFF + ((i + 1) << 45))
        if i in (79, 80):
            out.append((1.0, 0.0, 0.0, lo, hi))
            continue
        c = (Decimal(lo) + Decimal(hi)) / 2
        invc = rn(1 / c)
        lh, ll = dd(-Decimal(invc).ln())
        out.append((invc, lh, ll, lo, hi))
    return out


def main():
    ln2 = Decimal(2).ln()
    bits = struct.unpack("<Q", struct.pack("<d", rn(ln2)))[0] & ~((1 << 11) - 1)
    ln2hi = dbl(bits)                       # 42 significant bits: k * ln2hi is exact for |k| < 2^11
    ln2lo = rn(ln2 - Decimal(ln2hi))
    print(f"constexpr double kLn2Hi = {ln2hi.hex()}, kLn2Lo = {ln2lo.hex()};")
    worst = 0
    print("constexpr double kLogTab[128][3] = {")
    for invc, lh, ll, lo, hi in entries():
        for z in (Decimal(lo), Decimal(hi)):
            worst = max(worst, abs(z * Decimal(invc) - 1))
        print(f"    {{ {invc.hex()}, {lh.hex()}, {ll.hex()} }},")
    print("};")
    print(f"// max |z invc - 1| over the table: {float(worst):.6g} (2^-7 = {2.0 ** -7:.6g})")


if __name__ == "__main__":
    main()
