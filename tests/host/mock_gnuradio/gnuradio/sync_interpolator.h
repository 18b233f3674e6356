#ifndef MOCK_GR_SYNC_INTERPOLATOR_H
#define MOCK_GR_SYNC_INTERPOLATOR_H
// gr::sync_interpolator as far as the reference's unpack blocks need it (tests/golden/make_golden_packed.py drives them): work() over noutput_items
// outputs, noutput_items / interpolation inputs consumed
#include "gnuradio/sync_block.h"
namespace gr
{
class sync_interpolator : public sync_block
{
public:
    int general_work(int noutput_items, gr_vector_int&, gr_vector_const_void_star& input_items, gr_vector_void_star& output_items) override
    {
        const int n = work(noutput_items, input_items, output_items);
        if (n > 0) consume_each(n / static_cast<int>(d_interpolation));
        return n;
    }
    unsigned interpolation() const { return d_interpolation; }

protected:
    sync_interpolator(const std::string& name, io_signature::sptr in, io_signature::sptr out, unsigned interpolation)
        : sync_block(name, std::move(in), std::move(out)), d_interpolation(interpolation) {}
    unsigned d_interpolation;
};
}  // namespace gr
#endif
