"""The work-plane sizes of the depression-filling, drainage-area, watershed and stream-order entries, as a table: the layout
functions of nz_terrain_stages.cpp count tiles through csrc/nz_tile64.hpp, and a caller's allocation must not move with a
refactor of either.  The values are those the library returned when the tile size was still written as literals in the
host file; those of the watershed, stream-order and drainage-stripe entries are what it returned when each stage still had
a layout struct of its own."""
import ctypes as C

import noize_job_amd as nj

# (resolution, count, nz_fill_depressions_work_floats, nz_drainage_area_work_floats)
TILE = [
    (1, 1, 26, 29), (1, 3, 30, 31), (63, 1, 7962, 4989),
    (63, 3, 23838, 14911), (64, 1, 8216, 5144), (64, 3, 24600, 15384),
    (65, 1, 8474, 5309), (65, 3, 25382, 15879), (97, 1, 18842, 11789),
    (97, 3, 56494, 35327), (160, 1, 51232, 32032), (160, 3, 153664, 96064),
    (1024, 1, 2097680, 1311248), (1024, 3, 6293008, 3933712), (4096, 1, 33562640, 20979728),
    (4096, 3, 100687888, 62939152)]
# (cols, owned rows, pitch (0: cols), nz_fill_stripe_work_floats) of a stripe with one ghost row on each side
STRIPE = [
    (70, 1, 0, 234), (70, 1, 75, 249), (70, 16, 0, 1284), (70, 16, 75, 1374),
    (70, 17, 0, 1354), (70, 17, 75, 1449), (70, 200, 0, 14172), (70, 200, 75, 15182),
    (333, 1, 0, 1023), (333, 1, 338, 1038), (333, 16, 0, 6018), (333, 16, 338, 6108),
    (333, 17, 0, 6351), (333, 17, 338, 6446), (333, 200, 0, 67322), (333, 200, 338, 68332)]

# (resolution, count, nz_watershed_work_floats without and with a length, nz_stream_order_work_floats without and with links)
TILE_PAIRS = [
    (1, 1, 29, 30, 32, 33), (1, 3, 31, 34, 32, 35), (63, 1, 4989, 8958, 2016, 5985),
    (63, 3, 14911, 26818, 5984, 17891), (64, 1, 5144, 9240, 2072, 6168), (64, 3, 15384, 27672, 6168, 18456),
    (65, 1, 5309, 9534, 2144, 6369), (65, 3, 15879, 28554, 6376, 19051), (97, 1, 11789, 21198, 4736, 14145),
    (97, 3, 35327, 63554, 14160, 42387), (160, 1, 32032, 57632, 12832, 38432), (160, 3, 96064, 172864, 38464, 115264),
    (1024, 1, 1311248, 2359824, 524816, 1573392), (1024, 3, 3933712, 7079440, 1574416, 4720144),
    (4096, 1, 20979728, 37756944, 8396816, 25174032), (4096, 3, 62939152, 113270800, 25190416, 75522064)]
# (cols, owned rows, pitch (0: cols), nz_drainage_stripe_work_floats) of the same stripes
DRAINAGE_STRIPE = [
    (70, 1, 0, 290), (70, 1, 75, 309), (70, 16, 0, 1600), (70, 16, 75, 1714),
    (70, 17, 0, 1690), (70, 17, 75, 1809), (70, 200, 0, 17708), (70, 200, 75, 18970),
    (333, 1, 0, 1275), (333, 1, 338, 1294), (333, 16, 0, 7518), (333, 16, 338, 7632),
    (333, 17, 0, 7935), (333, 17, 338, 8054), (333, 200, 0, 84142), (333, 200, 338, 85404)]


def test_tile_entries_ask_for_what_they_asked_for():
    lib = nj._native.lib
    for res, count, fill, drainage in TILE:
        assert lib.nz_fill_depressions_work_floats(res, count) == fill, (res, count)
        assert lib.nz_drainage_area_work_floats(res, count) == drainage, (res, count)


def test_the_stripe_entry_asks_for_what_it_asked_for():
    lib = nj._native.lib
    for cols, own, pitch, want in STRIPE:
        st = nj._native.Stripe(cols, own + 2, 10, 1000, 1, 1 + own, pitch)
        assert lib.nz_fill_stripe_work_floats(C.byref(st)) == want, (cols, own, pitch)


def test_the_two_plane_entries_ask_for_what_they_asked_for():
    lib = nj._native.lib
    assert [t[:2] for t in TILE_PAIRS] == [t[:2] for t in TILE]
    for res, count, labels, with_length, orders, with_links in TILE_PAIRS:
        assert lib.nz_watershed_work_floats(res, count, 0) == labels, (res, count)
        assert lib.nz_watershed_work_floats(res, count, 1) == with_length, (res, count)
        assert lib.nz_stream_order_work_floats(res, count, 0) == orders, (res, count)
        assert lib.nz_stream_order_work_floats(res, count, 1) == with_links, (res, count)


def test_the_drainage_stripe_entry_asks_for_what_it_asked_for():
    lib = nj._native.lib
    assert [t[:3] for t in DRAINAGE_STRIPE] == [t[:3] for t in STRIPE]
    for cols, own, pitch, want in DRAINAGE_STRIPE:
        st = nj._native.Stripe(cols, own + 2, 10, 1000, 1, 1 + own, pitch)
        assert lib.nz_drainage_stripe_work_floats(C.byref(st)) == want, (cols, own, pitch)
