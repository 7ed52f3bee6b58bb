"""Textual-header helpers that step 8 needs (the reference keeps them in functions/header.py), on plain files with the standard library; and
the coordinate-scalar rule of step 16 (NumPy only for reading the first coordinate); and the scaling of header coordinates that steps 2 and 6
share (`scale_coordinates`, `unscale_coordinates`, as in the reference's functions/header.py).

A SEG-Y textual header is 3200 characters: 40 cards of 80, each opening with a 3-character label ('C 1' ... 'C40').  Processing steps are
logged as cards of the form ' YYYY-MM-DD: STEP' below a centred title card '***** PROCESSING WORKFLOW *****' (card 25 unless it exists elsewhere)."""
import datetime
import warnings

import numpy as np

from .segy import field_at

CARDS, WIDTH, LABEL = 40, 80, 3
TITLE = '***** PROCESSING WORKFLOW *****'
FULL = 'SEG-Y textual header is already full. Adding more information is not possible.'
# 1-based bytes of the x / y words the step CLIs' `--src_coords` / `--dst_coords` choose among
TRACE_HEADER_COORDS = {'source': (73, 77), 'CDP': (181, 185), 'group': (81, 85)}
COORDS = ['source', 'CDP', 'group']
ARC_SECONDS = 3600000
MSG_FORCED = 'Forced source CRS to be geographic (WGS84 - EPSG:4326)!'


def _cards(txt):
    """The header as a list of cards, from a newline-joined string or a list."""
    if isinstance(txt, str):
        return txt.split('\n')
    if isinstance(txt, list):
        return list(txt)
    raise ValueError(f'Not supported textual header type: {type(txt)}')


def _blank(card):
    return not card[LABEL:].strip() and len(card) == WIDTH


def _body(card, text):
    """``card`` with everything behind its label replaced by ``text``, padded to the card width."""
    return (card[:LABEL] + text).ljust(WIDTH)


def _codec(raw):
    """'ascii' or 'cp500' (EBCDIC).  Bytes outside ASCII are EBCDIC; so is a header without a single ASCII blank that holds EBCDIC
    blanks (0x40, '@' in ASCII): an empty EBCDIC header is all 0x40 and would otherwise pass for ASCII text."""
    if raw.isascii() and (b' ' in raw or b'@' not in raw):
        return 'ascii'
    return 'cp500'


def get_textual_header(path):
    """The textual header of a SEG-Y file as 40 newline-joined cards, decoded as ASCII or EBCDIC (code page 500; `_codec`)."""
    with open(path, 'rb') as fh:
        raw = fh.read(CARDS * WIDTH)
    text = raw.decode(_codec(raw))
    return '\n'.join(text[k:k + WIDTH] for k in range(0, len(text), WIDTH))


def _place_title(cards, title, card_no, overwrite):
    """Index of the card that holds ``title``: where it already stands, else card ``card_no`` (1-based), which is overwritten -- with
    a warning when it held text -- and the cards below it up to card 39 are blanked."""
    for k, card in enumerate(cards):
        if title in card:
            return k
    k = card_no - 1
    if not _blank(cards[k]):
        if not overwrite:
            raise Exception(f'Selected header line ({card_no}) is already in use and overwrite is set False.')
        warnings.warn('Selected header line is already in use and will be overwritten!', UserWarning)
    cards[k] = _body(cards[k], title.center(WIDTH - LABEL))
    for below in range(k + 1, CARDS - 1):
        cards[below] = _body(cards[below], '')
    return k


def add_processing_info_header(txt, info_str, prefix=None, header=True, header_line=25, overwrite=True, newline=False):
    """Log ``info_str`` in the textual header and return the new header string.

    With a ``prefix`` and ``newline`` False the text is appended (two blanks apart) to the first card below the title card that starts
    with the prefix and has room; otherwise it goes as ' prefix: info_str' (or the bare text without a prefix) onto the first blank card
    below the title card.  ``prefix`` '_TODAY_' / '_DATE_' stands for today's date.  ``header`` True selects the default title card, a
    string a custom one (``header_line``, ``overwrite``: where it is put when it does not exist yet)."""
    if header is not True and not isinstance(header, str):
        raise ValueError(f'Parameter < {header} > is not permitted as input for `header`')
    if isinstance(prefix, str) and prefix.upper() in ('_TODAY_', '_DATE_'):
        prefix = datetime.date.today().isoformat()
    cards = _cards(txt)
    title_at = _place_title(cards, TITLE, header_line, True) if header is True else _place_title(cards, header, header_line, overwrite)
    if not any(_blank(c) for c in cards):
        raise IndexError(FULL)

    if prefix is not None and not newline:
        for k in range(title_at + 1, len(cards)):
            used = len(cards[k].rstrip())
            if cards[k][LABEL + 1:].startswith(prefix) and len(info_str) < WIDTH - used:
                cards[k] = (cards[k][:used] + '  ' + info_str).ljust(WIDTH)[:WIDTH]
                return '\n'.join(cards)
    free = next((k for k in range(title_at + 1, len(cards)) if _blank(cards[k])), None)
    if free is None:
        raise IndexError(FULL)
    cards[free] = _body(cards[free], info_str if prefix is None else f' {prefix}: {info_str}')
    total = sum(len(c) for c in cards)
    assert total == CARDS * WIDTH, f'Length of updated textual header ({total}) is not correct ({CARDS * WIDTH} characters)'
    return '\n'.join(cards)


def write_textual_header(path, txt, **kwargs_segy):
    """Write the textual header (newline-joined cards or a list of cards, each cut to 80 characters) into the SEG-Y file at ``path``, in
    the encoding the file already uses (ASCII or EBCDIC)."""
    flat = ''.join(card[:WIDTH] for card in _cards(txt))[:CARDS * WIDTH].ljust(CARDS * WIDTH)
    with open(path, 'r+b') as fh:
        codec = _codec(fh.read(CARDS * WIDTH))
        fh.seek(0)
        fh.write(flat.encode(codec, 'replace'))


def check_coordinate_scalar(coord_scalar, xcoords=None, ycoords=None):
    """The coordinate scalar for header word 71 and the factor the coordinates are multiplied by before they are stored, ``(scalar, factor)``.

    A negative scalar means "divide on reading": factor = |scalar|; a positive one "multiply on reading": factor = 1 / scalar; 0 and ``None``
    give (0, 1).  'auto' fills the ten digits of a 32-bit word: with n characters in front of the decimal point of the first x or y coordinate
    as ``str`` prints it (the longer of the two; a minus sign counts, as in the reference), factor = 10^(9 - n), scalar = -factor, or
    int(1 / factor) where the factor is 1 or less."""
    if coord_scalar is None:
        coord_scalar = 0
    if isinstance(coord_scalar, str):
        if coord_scalar != 'auto':
            raise ValueError(f"coordinate scalar {coord_scalar!r}: an integer or 'auto'")
        ndigits = max(str(np.asarray(c).flat[0]).find('.') for c in (xcoords, ycoords))
        factor = 10 ** (9 - ndigits)
        return (-factor if factor > 1 else int(1 / factor)), factor
    if coord_scalar > 0:
        return coord_scalar, 1 / abs(coord_scalar)
    if coord_scalar < 0:
        return coord_scalar, abs(coord_scalar)
    return coord_scalar, 1


def scale_coordinates(segy, src_coords_bytes=(73, 77)):
    """(x, y, CoordinateUnits): the header coordinates at ``src_coords_bytes`` in their real unit.  The FIRST trace decides for all: units 1
    (length) apply its ``SourceGroupScalar`` (negative: divide by its magnitude, positive: multiply, 0: as stored), units 2 (seconds of arc)
    divide by 3 600 000; units 3 and 4 are not implemented (reference: functions/header.py ``scale_coordinates``).  This is reprojection's rule;
    `functions.segy.scaled_coordinates` is binning's, where a scalar of 0 gives 0 and the units are not looked at."""
    units = int(segy.header('CoordinateUnits')[0])
    x, y = segy.header(field_at(src_coords_bytes[0])), segy.header(field_at(src_coords_bytes[1]))
    if units == 1:
        scalar = int(segy.header('SourceGroupScalar')[0])
        if scalar < 0:
            x, y = x / np.abs(scalar), y / np.abs(scalar)
        elif scalar > 0:
            x, y = x * np.abs(scalar), y * np.abs(scalar)
    elif units == 2:
        x, y = x / ARC_SECONDS, y / ARC_SECONDS
    elif units == 3:
        raise NotImplementedError('Functionality to convert DD data is not implemented.')
    elif units == 4:
        raise NotImplementedError('Functionality to convert DMS data is not implemented.')
    return x, y, units


def unscale_coordinates(x, y, scale_factor=-100):
    """Coordinates in metres as the integers of a header with scalar ``scale_factor``: rounded ``v * |scalar|`` for a negative scalar,
    rounded ``v / |scalar|`` for a positive one, rounded ``v`` for 0 (reference: functions/header.py ``unscale_coordinates``, units 1).  The
    inverse of `scale_coordinates` (reprojection's rule), not of `functions.segy.scaled_coordinates` (binning's)."""
    x, y = np.asarray(x), np.asarray(y)
    if scale_factor < 0:
        x, y = x * np.abs(scale_factor), y * np.abs(scale_factor)
    elif scale_factor > 0:
        x, y = x / np.abs(scale_factor), y / np.abs(scale_factor)
    return np.around(x, 0).astype(np.int64), np.around(y, 0).astype(np.int64)
