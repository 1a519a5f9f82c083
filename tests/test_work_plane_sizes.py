"""The work-plane sizes of the depression-filling and drainage-area entries, as a table: the layout functions of
nz_terrain_stages.cpp count tiles through csrc/nz_tile64.hpp, and a caller's allocation must not move with a refactor of
either.  The values are those the library returned when the tile size was still written as literals in the host file."""
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
