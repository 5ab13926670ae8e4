// Stand-alone check of PageFeed (page_feed.h) without a device: tests/test_cli_page_feed_host.py builds it under the
// sanitizers and runs it.
//
//   page_feed_check PAGE_DIR OUT_DIR N_PAGES p0,n,w,h [p0,n,w,h ...]
//
// PAGE_DIR holds p00.pgm ... (binary PGM, page i filled with (i * 7 + row + col) & 255); the batches on the command
// line are what the plan must be for batch_pages = 4.  Exit 0: every check passed.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include <sys/stat.h>

#include "page_feed.h"

namespace {

#define CHECK(cond, ...)                                       \
    do {                                                       \
        if (!(cond)) {                                         \
            fprintf(stderr, "%s:%d: %s: ", __FILE__, __LINE__, #cond); \
            fprintf(stderr, __VA_ARGS__);                      \
            fputc('\n', stderr);                               \
            exit(1);                                           \
        }                                                      \
    } while (0)

const size_t BATCH_PAGES = 4, BAD_PAGE = 20;

uint8_t pattern(size_t page, size_t row, size_t col) { return (uint8_t)((page * 7 + row + col) & 255); }

void write_page(const std::string &path, size_t page, size_t w, size_t h, size_t drop_bytes) {
    std::vector<uint8_t> px(w * h);
    for (size_t r = 0; r < h; r++)
        for (size_t c = 0; c < w; c++) px[r * w + c] = pattern(page, r, c);
    FILE *f = fopen(path.c_str(), "wb");
    CHECK(f, "cannot write %s", path.c_str());
    fprintf(f, "P5\n%zu %zu\n255\n", w, h);
    fwrite(px.data(), 1, px.size() - drop_bytes, f);
    fclose(f);
}

void check_slab(const PageFeed::Batch &B, const uint8_t *slab) {
    for (size_t k = 0; k < B.n; k++)
        for (size_t r = 0; r < B.h; r++)
            for (size_t c = 0; c < B.w; c++)
                CHECK(slab[k * B.w * B.h + r * B.w + c] == pattern(B.p0 + k, r, c), "page %zu row %zu col %zu", B.p0 + k, r, c);
}

}  // namespace

int main(int argc, char **argv) {
    CHECK(argc > 4, "usage: page_feed_check PAGE_DIR OUT_DIR N_PAGES p0,n,w,h ...");
    const std::string page_dir = argv[1], out_dir = argv[2];
    const size_t n_pages = strtoul(argv[3], nullptr, 10);
    std::vector<PageFeed::Batch> want;
    for (int a = 4; a < argc; a++) {
        PageFeed::Batch B;
        CHECK(sscanf(argv[a], "%zu,%zu,%zu,%zu", &B.p0, &B.n, &B.w, &B.h) == 4, "bad batch '%s'", argv[a]);
        want.push_back(B);
    }
    std::vector<std::string> paths(n_pages), pngs(n_pages);
    for (size_t i = 0; i < n_pages; i++) {
        char name[32];
        snprintf(name, sizeof name, "/p%02zu", i);
        paths[i] = page_dir + name + ".pgm";
        pngs[i] = out_dir + name + ".png";
    }

    {  // pass 1: the plan, a ring that grows while the workers run and then wraps, PNG jobs between the decodes
        PageFeed feed(paths, BATCH_PAGES, 3, true);
        std::string e = feed.plan();
        CHECK(e.empty(), "plan: %s", e.c_str());
        CHECK(feed.n_batches() == want.size(), "%zu batches, expected %zu", feed.n_batches(), want.size());
        bool split_on_cap = false, split_on_size = false;
        size_t max_bytes = 0;
        for (size_t b = 0; b < want.size(); b++) {
            const PageFeed::Batch &B = feed.batch(b);
            CHECK(B.p0 == want[b].p0 && B.n == want[b].n && B.w == want[b].w && B.h == want[b].h, "batch %zu is %zu,%zu,%zu,%zu", b, B.p0, B.n, B.w, B.h);
            if (b && feed.batch(b - 1).n == BATCH_PAGES && feed.batch(b - 1).w == B.w && feed.batch(b - 1).h == B.h) split_on_cap = true;
            if (b && feed.batch(b - 1).n < BATCH_PAGES && (feed.batch(b - 1).w != B.w || feed.batch(b - 1).h != B.h)) split_on_size = true;
            max_bytes = std::max(max_bytes, B.n * B.w * B.h);
        }
        CHECK(split_on_cap && split_on_size, "the pages do not split a batch on the cap and on a size change");
        CHECK(feed.slab_bytes() >= max_bytes && feed.slab_bytes() % 4096 == 0, "slab of %zu bytes for batches of %zu", feed.slab_bytes(), max_bytes);
        e = feed.start(2);
        CHECK(e.empty(), "start: %s", e.c_str());
        e = feed.grow(3);
        CHECK(e.empty(), "grow: %s", e.c_str());
        CHECK(feed.slabs().size() == 3, "%zu slabs", feed.slabs().size());
        for (size_t b = 0; b < feed.n_batches(); b++) {
            const PageFeed::Batch &B = feed.batch(b);
            const PageFeed::Decoded d = feed.wait_decoded(b);
            CHECK(d.err.empty(), "batch %zu: %s", b, d.err.c_str());
            CHECK(d.slab == feed.slabs()[b % 3], "batch %zu is not in slab %zu", b, b % 3);
            check_slab(B, d.slab);
            e = feed.png_throttle(4);
            CHECK(e.empty(), "cannot write %s", e.c_str());
            auto rgb = std::make_shared<std::vector<uint8_t>>(B.n * B.w * B.h * 3);
            for (size_t q = 0; q < B.n * B.w * B.h; q++) (*rgb)[3 * q] = (*rgb)[3 * q + 1] = (*rgb)[3 * q + 2] = d.slab[q];
            feed.queue_pngs(std::vector<std::string>(pngs.begin() + B.p0, pngs.begin() + B.p0 + B.n), rgb, B.w, B.h);
            feed.retired(b);
        }
        e = feed.close_pngs();
        CHECK(e.empty(), "cannot write %s", e.c_str());
        feed.stop();
        for (const std::string &p : pngs) {
            struct stat st;
            CHECK(stat(p.c_str(), &st) == 0 && st.st_size > 0, "%s was not written", p.c_str());
        }
    }

    {  // pass 2: a page that cannot be decoded is reported with its batch; the batches before it still arrive
        size_t bad_batch = 0;
        while (want[bad_batch].p0 + want[bad_batch].n <= BAD_PAGE) bad_batch++;
        std::vector<std::string> with_bad = paths;  // the truncated page is a file of its own: PAGE_DIR stays as it was given
        with_bad[BAD_PAGE] = out_dir + "/truncated.pgm";
        write_page(with_bad[BAD_PAGE], BAD_PAGE, want[bad_batch].w, want[bad_batch].h, 5);
        PageFeed feed(with_bad, BATCH_PAGES, 3, false);
        std::string e = feed.plan();
        CHECK(e.empty(), "plan: %s", e.c_str());
        e = feed.start(2);
        CHECK(e.empty(), "start: %s", e.c_str());
        for (size_t b = 0; b < bad_batch; b++) {
            const PageFeed::Decoded d = feed.wait_decoded(b);
            CHECK(d.err.empty(), "batch %zu: %s", b, d.err.c_str());
            check_slab(feed.batch(b), d.slab);
            feed.retired(b);
        }
        const PageFeed::Decoded d = feed.wait_decoded(bad_batch);
        CHECK(d.err.find("truncated") != std::string::npos, "batch %zu: '%s'", bad_batch, d.err.c_str());
        feed.stop();  // with pages still to decode and batches not retired
        remove(with_bad[BAD_PAGE].c_str());
    }

    {  // pass 3: the ring refuses to grow once a batch beyond its first lap was given a slab
        PageFeed feed(paths, BATCH_PAGES, 3, false);
        std::string e = feed.plan();
        CHECK(e.empty(), "plan: %s", e.c_str());
        e = feed.start(2);
        CHECK(e.empty(), "start: %s", e.c_str());
        (void)feed.wait_decoded(0);
        feed.retired(0);
        (void)feed.wait_decoded(2);  // batch 2 went into batch 0's slab: slabs[2 % 2]
        e = feed.grow(3);
        CHECK(!e.empty(), "the ring grew from 2 to 3 slabs with batch 2 decoded into slab 0");
        CHECK(feed.slabs().size() == 2, "%zu slabs after the refused grow", feed.slabs().size());
        const PageFeed::Decoded d = feed.wait_decoded(1);
        check_slab(feed.batch(1), d.slab);
        check_slab(feed.batch(2), feed.wait_decoded(2).slab);
    }
    puts("page feed ok");
    return 0;
}
