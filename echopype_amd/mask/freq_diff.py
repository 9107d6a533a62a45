"""Host side of mask.frequency_differencing: the criterion string and the checks of the dataset it is applied to
(behaviour, error types and messages of the reference's mask/freq_diff.py)."""
import re

_OPERATORS = (">", "<", "<=", ">=", "==")
_UNIT = {"": 1, "k": 1e3, "M": 1e6, "G": 1e9}
_NUMBER = r"\d*\.?\d+"
# "<A> - <B> <operator> <number> dB": the operator is whatever non-blank text stands between B and the number
_TAIL = r"\s*(?P<op>\S*?)\s*(?P<db>" + _NUMBER + r")\s*dB"
_FREQ_EQ = re.compile(r"(?P<a>" + _NUMBER + r")\s*(?P<ua>\w?)Hz\s*-\s*(?P<b>" + _NUMBER + r")\s*(?P<ub>\w?)Hz" + _TAIL)
_CHAN_EQ = re.compile(r'(?P<a>".+")\s*-\s*(?P<b>".+")\s*' + _TAIL)


def _parse_freq_diff_eq(freqABEq=None, chanABEq=None):
    """``[freqAB, chanAB, operator, diff]`` of a criterion such as ``"38.0kHz - 120 kHz >= 10.0dB"`` (``freqABEq``:
    frequencies in Hz with the prefixes "", k, M, G) or ``'"chan1" - "chan2" < 5dB'`` (``chanABEq``: channel names in
    double quotes).  Exactly one of the two is given; the one not given comes back as None, ``diff`` as a float."""
    if freqABEq is None and chanABEq is None:
        raise ValueError("Either freqAB or chanAB must be given!")
    if freqABEq is not None and chanABEq is not None:
        raise ValueError("Only one of freqAB or chanAB should be given, but not both!")
    by_freq = freqABEq is not None
    m = (_FREQ_EQ if by_freq else _CHAN_EQ).match(freqABEq if by_freq else chanABEq)
    if m is None:
        raise TypeError(f"Invalid {'freqAB' if by_freq else 'chanAB'} Equation!")
    if m["op"] not in _OPERATORS:
        raise ValueError("Invalid operator!")
    if by_freq:
        # (a prefix outside the table is a KeyError, as in the reference)
        pair = [float(m["a"]) * _UNIT[m["ua"]], float(m["b"]) * _UNIT[m["ub"]]]
    else:
        pair = [m["a"][1:-1], m["b"][1:-1]]
    if len(set(pair)) != 2:
        raise ValueError(f"{'freqAB' if by_freq else 'chanAB'} must be a list of length 2 with unique elements!")
    diff = float(m["db"])
    return [pair, None, m["op"], diff] if by_freq else [None, pair, m["op"], diff]


def _check_freq_diff_source_Sv(source_Sv, freqAB=None, chanAB=None):
    """``source_Sv`` has the coordinate ``channel`` and the variable ``frequency_nominal``; the one the criterion
    selects by holds no repeated values and holds both selected values."""
    if "channel" not in source_Sv.coords:
        raise ValueError("The Dataset defined by source_Sv must have channel as a coordinate!")
    if "frequency_nominal" not in source_Sv.variables:
        raise ValueError("The Dataset defined by source_Sv must have frequency_nominal as a variable!")
    if chanAB is not None:
        channels = list(source_Sv["channel"].values)
        if len(set(channels)) < len(channels):
            raise ValueError("The provided source_Sv contains repeated channel values, this is not allowed!")
        if not all(chan in channels for chan in chanAB):
            raise ValueError("The provided list input chanAB contains values that are not in the channel coordinate!")
    if freqAB is not None:
        freqs = list(source_Sv["frequency_nominal"].values)
        if len(set(freqs)) < len(freqs):
            raise ValueError("The provided source_Sv contains repeated frequency_nominal values, this is not allowed!")
        if not all(freq in freqs for freq in freqAB):
            raise ValueError("The provided list input freqAB contains values that are not in the frequency_nominal "
                             "variable!")
