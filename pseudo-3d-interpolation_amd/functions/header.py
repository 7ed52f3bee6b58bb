"""Textual-header helpers that step 8 needs (the reference keeps them in functions/header.py), on plain files with the standard library; and
the coordinate-scalar rule of step 16 (NumPy only for reading the first coordinate).

A SEG-Y textual header is 3200 characters: 40 cards of 80, each opening with a 3-character label ('C 1' ... 'C40').  Processing steps are
logged as cards of the form ' YYYY-MM-DD: STEP' below a centred title card '***** PROCESSING WORKFLOW *****' (card 25 unless it exists elsewhere)."""
import datetime
import warnings

import numpy as np

CARDS, WIDTH, LABEL = 40, 80, 3
TITLE = '***** PROCESSING WORKFLOW *****'
FULL = 'SEG-Y textual header is already full. Adding more information is not possible.'


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
